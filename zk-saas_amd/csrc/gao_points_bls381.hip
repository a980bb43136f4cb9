// zk_pss_unpack_points_robust, zk_pss_repair_points and their _parties forms over G1 and G2 of this curve (gao_points_impl.hpp).
// a 12-limb base field: inline products, so that the G1 kernels keep out of scratch memory (field.hpp ZK_MUL_INLINE_LIMBS)
#define ZK_MUL_INLINE_LIMBS 12
#include "curves.hpp"
#include "gao_points_impl.hpp"

namespace zk {
#define GAO_PT_INST(FR, FLD, RE)                                                                                          \
  template int gao_points_run<FR, FLD, RE>(IEngine*, DevBuf&, int, std::conditional_t<RE, void*, const void*>, size_t, int, \
                                           const GaoPtTable<Fp<FR>>*, const Fp<FR>*, const GaoPtList<Fp<FR>>*, void*, uint8_t*,  \
                                           uint32_t*, uint64_t*, hipStream_t);
GAO_PT_INST(Bls381Fr, Fp<Bls381Fq>, false)
GAO_PT_INST(Bls381Fr, Fp<Bls381Fq>, true)
GAO_PT_INST(Bls381Fr, Fp2<Bls381Fq>, false)
GAO_PT_INST(Bls381Fr, Fp2<Bls381Fq>, true)
#undef GAO_PT_INST
}  // namespace zk
