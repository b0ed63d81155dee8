/*
 * g4d_sets.h -- entry points of libg4d_hip.so that came after the record of g4d.h was closed: a further header of the SAME library (no
 * library of its own; garment4d_amd/_lib.py reads it with the parse it reads g4d.h with, sets_lib(); record: tests/sets_abi_snapshot.txt).
 * The boundary contract of g4d.h holds unchanged: raw device pointers + sizes + a HIP stream, status codes, g4d_last_error().
 */
#ifndef G4D_SETS_H
#define G4D_SETS_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* g4d_ball_grid_query_f32 (same arguments, same grid) for consumers that reduce over a neighbourhood with an order-independent operation (the
 * max-pooled set-abstraction kernels): per (query, scale) the slots hold the SAME SET of indices as the ordered form -- the nsample smallest
 * indices of the ball when it holds more -- each once, in unspecified order; padding slots repeat slot 0; a row without hits is zeros.
 * Saves the ordered form's rank pass. */
int g4d_ball_grid_query_set_f32(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *new_xyz,
                                const float *xyz, int *const *idx, const void *grid, float grid_rmax, g4d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G4D_SETS_H */
