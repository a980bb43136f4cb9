// The chunk ranges of the all-to-all king (engine_dist.inc.hpp king_round_a2a) and the column -> chunk map of a rank's
// [np][seg] block, in one place for the host and the device: a2a_plan cuts the ranges with king_span, the range form of the
// repair (gao_impl.hpp) writes status and errpos at king_chunk.  Plain integers only: this header compiles for the host alone
// (tests/native/king_range_host_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZK_KR_HD __host__ __device__ __forceinline__
#else
#define ZK_KR_HD inline
#endif

namespace zk {

// the share of present rank `me` (its index among the npresent present ranks) of `len` columns cut at multiples of `gran`:
// it owns [me * seg, (me + 1) * seg), of which [rs, rs + cnt) exist (cnt < seg for the last range, 0 beyond it)
struct KingSpan {
  uint32_t seg, rs, cnt;
};
// false when there is less than one granule per rank, len is no multiple of gran, or a range does not fit 32 bits
ZK_KR_HD bool king_span(size_t len, size_t gran, size_t npresent, size_t me, KingSpan* sp) {
  if (!gran || npresent < 2 || me >= npresent || len / gran < npresent || len % gran) return false;
  const size_t seg = ((len / gran + npresent - 1) / npresent) * gran;
  if (seg > 0xffffffffull) return false;
  const size_t rs0 = me * seg;
  sp->seg = (uint32_t)seg;
  sp->rs = (uint32_t)(rs0 < len ? rs0 : len);
  sp->cnt = (uint32_t)(rs0 >= len ? 0 : (len - rs0 < seg ? len - rs0 : seg));
  return true;
}
// the input chunk in column c of the block of the rank whose range starts at `base`: a2a_pack_kernel's
// (idx * seg + c - shift) mod len (pss.hpp; shift = 1 for d_fft, whose workgroup k0 reads the chunks k0 - 1 .. k0 + Wc - 2)
ZK_KR_HD uint32_t king_chunk(uint32_t base, uint32_t c, uint32_t len, uint32_t shift) {
  return (uint32_t)(((uint64_t)base + c + len - shift) % len);
}

// the same map with the offset folded in, for the kernels: off = king_chunk(base, 0, len, shift) < len and c < len, so one
// compare and one add or subtract take the place of the 64-bit remainder
ZK_KR_HD uint32_t king_chunk_from(uint32_t off, uint32_t c, uint32_t len) {
  const uint32_t room = len - off;       // columns before the wrap
  return c < room ? off + c : c - room;
}

// A word that lies in a block with padding: `cnt` valid columns of rows `stride` elements apart; column c is chunk
// king_chunk(base, c, len, shift) of the whole word.  stride == cnt == len, base == 0, shift == 0: the whole word.
struct GaoRange {
  size_t stride;
  uint32_t cnt, base, shift, len;
  ZK_KR_HD uint32_t chunk(uint32_t c) const { return king_chunk(base, c, len, shift); }
};

// what a kernel takes of a GaoRange: four words (the l = 8 scan has no scalar register to spare)
struct GaoRangeDev {
  uint32_t stride, cnt, off, len;
  ZK_KR_HD uint32_t chunk(uint32_t c) const { return king_chunk_from(off, c, len); }
};
// stride must fit 32 bits (the caller's check)
ZK_KR_HD GaoRangeDev gao_range_dev(const GaoRange& rg) {
  return GaoRangeDev{(uint32_t)rg.stride, rg.cnt, rg.len ? king_chunk(rg.base, 0, rg.len, rg.shift) : 0u, rg.len};
}

}  // namespace zk
