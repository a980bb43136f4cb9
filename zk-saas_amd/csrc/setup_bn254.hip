// zk_groth16_setup_scalars over the scalar field of this curve (setup_impl.hpp).
#include "curves.hpp"
#include "setup_impl.hpp"

namespace zk {
template int setup_scalars_run<Bn254Fr>(IEngine*, DevBuf&, const void* const[9], size_t, size_t, size_t, int, const void*, size_t,
                                   void* const[5], hipStream_t);
}  // namespace zk
