/*
 * g4d_live.h -- the live-cloud scope of libg4d_hip.so: a further header of the SAME library (no library of its own; garment4d_amd/_lib.py
 * reads it with the parse it reads g4d.h with, live_lib(); record: tests/live_abi_snapshot.txt).
 *
 * A caller that launches the hot path on a FIXED number of clouds (a captured hipGraph: grids and arguments are frozen) but has fewer clouds
 * to compute opens a scope around its launches:
 *
 *     g4d_live_scope_begin(count_dev, capacity);    count_dev: ONE int in device memory, read by the kernels when they RUN
 *     ... entry points of g4d.h / g4d_sets.h, called with b = capacity clouds ...
 *     g4d_live_scope_end();
 *
 * Inside the scope every converted entry point whose launch is provably cloud-major -- its `b` equals `capacity`, or, for an entry point that
 * takes rows only, its rows are a multiple of `capacity` -- hands {count_dev, capacity, rows per cloud} to its kernels.  Each kernel reads the
 * count once, clamps it to [0, capacity], and computes the first `count` clouds only: their results are the bits of a launch with b = count;
 * rows of the other clouds are neither read nor written.  Grids stay sized for `capacity`; surplus workgroups leave at once.  A launch that
 * is not provably cloud-major, and an entry point that is not converted, ignores the scope and computes everything.
 *
 * The scope is state of the calling OS thread (like g4d_tuning_set_thread): it applies to launches made, or captured, by that thread between
 * begin and end.  Scopes do not nest.  The count may be rewritten between replays of a captured graph, on the graph's stream.
 */
#ifndef G4D_LIVE_H
#define G4D_LIVE_H

#include "g4d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G4D_EINVAL: null pointer, capacity_clouds < 1, or a scope is already open on this thread. */
int g4d_live_scope_begin(const int *live_clouds_dev, int capacity_clouds);
/* G4D_EINVAL: no scope is open on this thread. */
int g4d_live_scope_end(void);
/* Capacity of the calling thread's open scope; 0: none is open. */
int g4d_live_scope_capacity(void);
/* What a converted launcher called now, on this thread, with `clouds` clouds (-1: an entry point that takes rows only) and `rows` rows in all
 * would hand to its kernel: the rows per cloud when the scope applies, 0 when the launch ignores it (no scope, clouds != capacity, rows not a
 * multiple of the capacity).  For tests: needs no GPU. */
long long g4d_live_scope_rows_per_cloud(long long clouds, long long rows);

#ifdef __cplusplus
}
#endif
#endif /* G4D_LIVE_H */
