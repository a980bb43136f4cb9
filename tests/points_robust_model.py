"""What zk_pss_unpack_points_robust and zk_pss_repair_points decide about a word of point shares Y_p = y_p G, stated on the
scalar word y: the verdict of the unchanged tests/gao_model.py, cut down to the one error per chunk that can be located in
the exponent.

TEST INFRASTRUCTURE ONLY.  Both decoders are exact bounded-distance decoders of the same code -- Gao's up to (n - k) // 2
wrong shares, the point form up to one (none when n - k = 1) -- so the point form's verdict follows from Gao's:
  Gao's status 0                            stays 0
  Gao's status 1 with one bit in errpos     stays 1 with that bit
  everything else                           is 2: message zeros, errpos 0
(A word one share away from a codeword has n - k >= 2, where Gao's cap is at least 1 and its status is 1 with that one bit;
a word Gao corrects in two or more places is not within one of any codeword, the minimum distance being n - k + 1.)"""
import gao_model as gm


def decode(y, k, omega, p):
    """-> gao_model.Decoded(status, message padded to k coefficients, errpos) under the rule above"""
    d = gm.decode(y, k, omega, p)
    if d.status == 0 or (d.status == 1 and bin(d.errpos).count("1") == 1):
        return d
    return gm.Decoded(2, [0] * k, 0)


def repaired(y, k, omega, p):
    """(Decoded, the word after zk_pss_repair_points): the codeword for status 1, y itself otherwise"""
    d = decode(y, k, omega, p)
    if d.status != 1:
        return d, list(y)
    return d, gm.encode(gm.trim(d.message), len(y), omega, p)
