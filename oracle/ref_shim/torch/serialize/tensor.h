/* Shadows <torch/serialize/tensor.h> for the `ref` target of oracle/Makefile: the reference's kernel headers also declare the
 * tensor-taking wrappers of its .cpp files, which this build neither compiles nor calls -- a forward declaration is all they need. */
#ifndef G4D_REF_SHIM_TORCH_SERIALIZE_TENSOR_H
#define G4D_REF_SHIM_TORCH_SERIALIZE_TENSOR_H
namespace at {
class Tensor;
}
#endif
