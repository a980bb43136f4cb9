"""fft1, d_fft and d_ifft at every transform size and pass shape (docs/ntt_size_tests.md).

csrc/ntt.hpp cuts the log_n stages of fft1 into passes (make_ntt_plan); every log_n from 8 to 20 gives another
(s0, s1, cbits) triple and with it other code in ntt_pass_kernel (odd / even prologue, whole rows or column tiles, stage
twiddles from LDS or from the full table), and king_fft2_kernel changes its block and LDS shape with Lc = m / l.  All
arithmetic is integer: every comparison is exact equality with the plain-C oracle (oracle/c/zkref.c), which
tests/test_oracle_c.py pins on the Python oracle.  tests/ntt_sizes.py holds the size grids; tests/test_ntt_plan.py checks
on the CPU that they reach every shape."""
import contextlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from oracle.cref import CPss
from oracle.field import Domain
from oracle.params import CURVES

import ntt_sizes as ns
from gpu_util import ctx

_CP = {}


def _cp(curve, l):
    if (curve, l) not in _CP:
        _CP[(curve, l)] = CPss(curve, l)
    return _CP[(curve, l)]


@contextlib.contextmanager
def _context(curve, l, log_m):
    """One context per (curve, l); from log_m = 24 up a context of its own that is closed afterwards, so that its cached
    twiddle tables (2^log_m + 1 elements per direction) are released."""
    if log_m < 24:
        yield ctx(curve, l)
        return
    pp = zk.PackedSharingParams(curve, l)
    try:
        yield pp
    finally:
        pp.close()


def _rand_fr_array(count, seed, top_bits=60):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << top_bits) - 1)        # < r for all three scalar fields: valid Montgomery residues
    return a


STRUCTURED = ("r-1", "zero", "const")


def _structured(cp, log_n):
    """The three structured vectors, at every size: all r - 1, all zero, a constant."""
    vals = {"r-1": cp.opp.p - 1, "zero": 0, "const": 0x1234567}
    return [np.tile(cp.fr.enc([vals[kind]]), (1 << log_n, 1)) for kind in STRUCTURED]


def _same(got, want, what, log_n=None):
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).any(axis=1))[0]
    where = ""
    if log_n is not None and ns.tile_bits(log_n):
        k = int(bad[0]) % (1 << log_n)
        where = "; vector %d, output %d; plan %s (pass 0 tile %d)" % (int(bad[0]) >> log_n, k, ns.plan(log_n),
                                                                      k >> ns.plan(log_n)[0][1])
    pytest.fail("%s: %d of %d elements differ, first at %d%s" % (what, bad.size, len(want), int(bad[0]), where))


def _fft1(pp, buf, log_m, inverse, batch, add=None):
    pp._check(pp.lib.zk_fft1(pp.h, buf.ptr, log_m, inverse, batch, None if add is None else add.ptr, None))


def _log2(l):
    return l.bit_length() - 1


# ------------------------------------------------------------------------------------------------ a. fft1, full output
@pytest.mark.parametrize("curve,l,log_n", ns.FFT1_FULL, ids=["%s-l%d-logn%02d" % c for c in ns.FFT1_FULL])
def test_fft1_full_output_equals_c_oracle(curve, l, log_n):
    """zk_fft1 on five different vectors at once (two dense random ones, then all r - 1, all zero and a constant; a
    blockIdx.y stride error shows), both directions: every output equals zkref_fft1's; once more with a random add_d:
    the reference plus that vector.  The all-zero input gives all zero, the other two do not."""
    log_m = log_n + _log2(l)
    n, batch = 1 << log_n, 5
    cp = _cp(curve, l)
    dom = Domain(CURVES[curve], 1 << log_m)
    x = np.concatenate([_rand_fr_array(n, 1000 + log_n), _rand_fr_array(n, 2000 + log_n)] + _structured(cp, log_n))
    add = _rand_fr_array(batch * n, 3000 + log_n)
    gens = (dom.group_gen, dom.group_gen_inv)
    with ThreadPoolExecutor(max_workers=2 * batch) as pool:      # the C calls release the GIL
        jobs = [[pool.submit(cp.fft1_arrays, x[b * n:(b + 1) * n].copy(), gens[inv]) for b in range(batch)]
                for inv in (0, 1)]
        want = [np.concatenate([j.result() for j in row]) for row in jobs]
    with _context(curve, l, log_m) as pp:
        add_d = zk.DeviceBuffer.from_numpy(pp, add)
        for inv in (0, 1):
            what = "fft1 %s l=%d log_n=%d inverse=%d" % (curve, l, log_n, inv)
            buf = zk.DeviceBuffer.from_numpy(pp, x)
            _fft1(pp, buf, log_m, inv, batch)
            got = buf.to_numpy().reshape(-1, 4)
            _same(got, want[inv], what, log_n)
            for i, kind in enumerate(STRUCTURED):
                assert got[(2 + i) * n:(3 + i) * n].any() == (kind != "zero"), (what, kind)
            buf.free()
            buf = zk.DeviceBuffer.from_numpy(pp, x)
            _fft1(pp, buf, log_m, inv, batch, add_d)
            _same(buf.to_numpy().reshape(-1, 4), cp.add_arrays(want[inv], add), what + " + add_d", log_n)
            buf.free()
        add_d.free()


# ------------------------------------------------------------------------------------------------ b. the largest sizes
SAMPLED_RUNS = [c + (inv,) for c in ns.FFT1_SAMPLED for inv in (0, 1)]


@pytest.mark.parametrize("curve,l,log_n,inverse", SAMPLED_RUNS, ids=["%s-l%d-logn%02d-inv%d" % c for c in SAMPLED_RUNS])
def test_fft1_largest_sizes_equal_the_closed_form_at_sampled_outputs(curve, l, log_n, inverse):
    """BN254, l = 2, log_n = 25, 26, 27 (log_m = 28 is the field's two-adicity): a dense random input; the outputs at a
    fixed-seed sample of 64 positions, at the first and last index of the first and last tile and on both sides of every
    pass's row boundary equal zkref_fft1_eval's (the closed form, no butterfly).  A size that cannot be allocated is
    skipped with the byte count."""
    log_m = log_n + _log2(l)
    n = 1 << log_n
    cp = _cp(curve, l)
    dom = Domain(CURVES[curve], 1 << log_m)
    ks = ns.sample_positions(log_n)
    assert len(ks) >= 64 and {0, 2047, n - 2048, n - 1} <= set(ks)
    assert all({(1 << s0) - 1, 1 << s0} <= set(ks) for s0, _s1, _cb in ns.plan(log_n))
    need = 32 * n + 32 * ((1 << log_m) + 1)            # the vector + the twiddle table of one direction
    try:
        x = _rand_fr_array(n, 4000 + log_n)
    except MemoryError:
        pytest.skip("2^%d: no %d bytes of host memory for the input" % (log_n, 32 * n))
    with _context(curve, l, log_m) as pp:
        # the only skip: the device cannot hold `need` bytes, asked with one allocation of that size before any work;
        # everything after it (upload, table build, the passes, the sync) fails the test when it raises
        try:
            probe = zk.DeviceBuffer(pp, need)
        except zk.ZkError as e:
            if e.msg != "hipMalloc: out of memory":
                raise
            pytest.skip("2^%d: no %d bytes of device memory" % (log_n, need))
        probe.free()
        buf = zk.DeviceBuffer.from_numpy(pp, x)
        _fft1(pp, buf, log_m, inverse, 1)
        pp.sync()
        got = np.stack([buf.view(32 * k, 32).to_numpy() for k in ks])
        buf.free()
    want = cp.fft1_eval_arrays(x, dom.group_gen_inv if inverse else dom.group_gen, ks, threads=16)
    bad = [k for k, g, w in zip(ks, got, want) if not np.array_equal(g, w)]
    assert not bad, "fft1 log_n=%d inverse=%d: %d of %d sampled outputs differ: %s; plan %s" % (
        log_n, inverse, len(bad), len(ks), bad[:12], ns.plan(log_n))


# ------------------------------------------------------------------------------------------------ c. rejections
@pytest.mark.parametrize("curve", ["bn254", "bls12_381", "bls12_377"])
def test_fft1_above_the_two_adicity_is_bad_input(curve):
    pp = ctx(curve, 2)
    buf = pp.alloc_fr(16)
    top = ns.TWO_ADICITY[curve]
    for inverse in (0, 1):
        with pytest.raises(zk.ZkError) as e:
            _fft1(pp, buf, top + 1, inverse, 1)
        assert e.value.code == 4
    _fft1(pp, buf, 4, 0, 2)                           # the context still works


@pytest.mark.parametrize("l", [2, 4, 8])
def test_fft1_with_log_m_below_log_l_is_bad_input(l):
    pp = ctx("bn254", l)
    buf = pp.alloc_fr(16)
    for log_m in range(_log2(l)):
        with pytest.raises(zk.ZkError) as e:
            _fft1(pp, buf, log_m, 0, 1)
        assert e.value.code == 4
    with pytest.raises(zk.ZkError) as e:
        _fft1(pp, buf, -1, 0, 1)
    assert e.value.code == 4


# ------------------------------------------------------------------------------------------------ d. d_fft / d_ifft
def _dfft_cases():
    """Main sweep: BN254, l = 2 (n = 8), every log_m from 1 to 22; boundary sizes: l = 1, 4, 8 at the log_m that put
    Lc = m / l at 32, 64, 128, 2^16 and 2^17.  (inverse, masked, rearrange) rotates WITHIN each king-block class
    (Lc < 64; 64 <= Lc <= 2^16; Lc > 2^16), so that all eight combinations appear in each."""
    sizes = [("bn254", 2, log_m) for log_m in range(1, 23)]
    sizes += [("bn254", l, log_lc + _log2(l)) for l in (1, 4, 8) for log_lc in (5, 6, 7, 16, 17)]
    seen, out = {}, []
    for curve, l, log_m in sizes:
        cls = ns.king_class((1 << log_m) // l)
        i = seen.get(cls, 0)
        seen[cls] = i + 1
        out.append((curve, l, log_m, i & 1, (i >> 1) & 1, (i >> 2) & 1))
    return out


DFFT_CASES = _dfft_cases()


def test_d_fft_cases_hold_all_eight_combinations_in_every_king_block_class():
    combos = {}
    for _c, l, log_m, inverse, masked, rearrange in DFFT_CASES:
        combos.setdefault(ns.king_class((1 << log_m) // l), set()).add((inverse, masked, rearrange))
    assert set(combos) == {"below64", "wave", "block"} and all(len(v) == 8 for v in combos.values()), combos
    assert {log_m for _c, l, log_m, *_ in DFFT_CASES if l == 2} == set(range(1, 23))


@pytest.mark.parametrize("curve,l,log_m,inverse,masked,rearrange", DFFT_CASES,
                         ids=["%s-l%d-logm%02d-inv%d-mask%d-rearr%d" % c for c in DFFT_CASES])
def test_d_fft_shares_equal_c_oracle(curve, l, log_m, inverse, masked, rearrange):
    """zk_d_fft / zk_d_ifft (coset g as groth16/src/ext_wit.rs:120-125): every output share equals the C oracle's, with
    FftMask::zero() or a sampled mask pair; then once more into out_d != shares_d: the same shares, and shares_d
    bit for bit as it was (include/zksaas.h)."""
    pp, cp = ctx(curve, l), _cp(curve, l)
    c = CURVES[curve]
    m = 1 << log_m
    mbyl = m // l
    dom = Domain(c, m)
    shares = _rand_fr_array(pp.n * mbyl, 5)
    g = Domain(c, 2 * m).element(1) if inverse else None
    mask, im, om = zk.FftMask.zero(), None, None
    if masked:
        mask = zk.FftMask.sample(pp, rearrange, g, inverse, log_m, 123)
        im = mask.in_mask.to_numpy().reshape(-1, 4).copy()
        om = mask.out_mask.to_numpy().reshape(-1, 4).copy()
        assert im.any() and om.any() and not np.array_equal(im, om)

    def run(buf, out):
        if inverse:
            zk.d_ifft(pp, buf, mask, rearrange, log_m, g=g, seed=77, out=out)
        else:
            zk.d_fft(pp, buf, mask, rearrange, log_m, seed=77, out=out)
    buf = zk.DeviceBuffer.from_numpy(pp, shares)
    run(buf, None)
    got = buf.to_numpy().reshape(-1, 4)
    want = shares.copy()
    ref = cp.d_fft_arrays_mt if log_m >= 18 else cp.d_fft_arrays
    kw = {"king_threads": 16} if log_m >= 18 else {}
    ref(want, mbyl, dom.group_gen_inv if inverse else dom.group_gen, dom.size_inv if inverse else None, g, rearrange,
        im, om, 77, **kw)
    what = "d_%sfft %s l=%d log_m=%d masked=%d rearrange=%d" % ("i" if inverse else "", curve, l, log_m, masked, rearrange)
    _same(got, want, what)
    src = zk.DeviceBuffer.from_numpy(pp, shares)
    out = zk.DeviceBuffer.from_numpy(pp, np.full_like(shares, 0xA5A5A5A5A5A5A5A5))
    run(src, out)
    _same(out.to_numpy().reshape(-1, 4), want, what + " (out_d)")
    assert np.array_equal(src.to_numpy().reshape(-1, 4), shares), what + ": shares_d changed"
    for b in (buf, src, out, mask.in_mask, mask.out_mask):
        if b is not None:
            b.free()
