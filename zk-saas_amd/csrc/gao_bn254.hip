// The error-correcting unpack and the repair over the scalar field of this curve: the one driver of gao_impl.hpp.
#include "curves.hpp"
#include "gao_impl.hpp"

namespace zk {
template int gao_run<Bn254Fr, false>(IEngine*, void*, int, const GaoCall&, hipStream_t);
template int gao_run<Bn254Fr, true>(IEngine*, void*, int, const GaoCall&, hipStream_t);
}  // namespace zk
