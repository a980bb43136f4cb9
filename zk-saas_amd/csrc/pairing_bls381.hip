// The verifier's kernels for BLS12-381 (pairing_impl.hpp), apart from the prover's translation units.
#include "pairing_impl.hpp"
#include "curves.hpp"
namespace zk {
IPairing* pairing_bls381() {
  static PairingImpl<PairingBls381, CfgBls381::FrP, ZK_BLS12_381, CfgBls381::B1> p;
  return &p;
}
}  // namespace zk
