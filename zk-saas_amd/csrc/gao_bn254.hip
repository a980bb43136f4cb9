// zk_pss_unpack_robust, zk_pss_unpack_robust_parties, zk_pss_repair, zk_pss_repair_parties, zk_pss_repair_batch, zk_pss_repair_batch_parties and the range form of the repair over the scalar field of this curve (gao_impl.hpp).
#include "curves.hpp"
#include "gao_impl.hpp"

namespace zk {
template int gao_unpack_robust_run<Bn254Fr>(IEngine*, DevBuf&, int, const void*, size_t, int, void*, void*, uint8_t*, uint32_t*,
                                       uint64_t*, hipStream_t);
template int gao_unpack_robust_parties_run<Bn254Fr>(IEngine*, DevBuf&, int, const void*, const uint32_t*, int, size_t, int, void*,
                                               void*, uint8_t*, uint32_t*, uint64_t*, hipStream_t);
template int gao_repair_run<Bn254Fr>(IEngine*, DevBuf&, int, void*, size_t, int, uint8_t*, uint32_t*, uint64_t*, hipStream_t);
template int gao_repair_parties_run<Bn254Fr>(IEngine*, DevBuf&, int, void*, const uint32_t*, int, size_t, int, uint8_t*, uint32_t*,
                                        uint64_t*, hipStream_t);
template int gao_repair_batch_run<Bn254Fr>(IEngine*, void*, int, void*, size_t, int, size_t, int, uint8_t*, uint32_t*, uint64_t*,
                                      hipStream_t);
template int gao_repair_batch_parties_run<Bn254Fr>(IEngine*, void*, int, void*, const uint32_t*, int, size_t, int, size_t, int, uint8_t*,
                                              uint32_t*, uint64_t*, hipStream_t);
template int gao_repair_range_run<Bn254Fr>(IEngine*, DevBuf&, int, void*, const uint32_t*, int, const GaoRange&, int, uint8_t*, uint32_t*,
                                      uint64_t*, hipStream_t);
}  // namespace zk
