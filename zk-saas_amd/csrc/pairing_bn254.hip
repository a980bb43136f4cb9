// The verifier's kernels for BN254 (pairing_impl.hpp), apart from the prover's translation units.
#include "pairing_impl.hpp"
#include "curves.hpp"
namespace zk {
IPairing* pairing_bn254() {
  static PairingImpl<PairingBn254, CfgBn254::FrP, ZK_BN254, CfgBn254::B1> p;
  return &p;
}
}  // namespace zk
