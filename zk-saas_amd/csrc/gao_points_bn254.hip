// zk_pss_unpack_points_robust, zk_pss_repair_points and their _parties forms over G1 and G2 of this curve (gao_points_impl.hpp).
#include "curves.hpp"
#include "gao_points_impl.hpp"

namespace zk {
#define GAO_PT_INST(FR, FLD, RE)                                                                                          \
  template int gao_points_run<FR, FLD, RE>(IEngine*, DevBuf&, int, std::conditional_t<RE, void*, const void*>, size_t, int, \
                                           const GaoPtTable<Fp<FR>>*, const Fp<FR>*, const GaoPtList<Fp<FR>>*, void*, uint8_t*,  \
                                           uint32_t*, uint64_t*, hipStream_t);
GAO_PT_INST(Bn254Fr, Fp<Bn254Fq>, false)
GAO_PT_INST(Bn254Fr, Fp<Bn254Fq>, true)
GAO_PT_INST(Bn254Fr, Fp2<Bn254Fq>, false)
GAO_PT_INST(Bn254Fr, Fp2<Bn254Fq>, true)
#undef GAO_PT_INST
}  // namespace zk
