"""zk_d_pp and zk_deg_red / zk_deg_red_parties at every packing factor, kernel choice and scan shape, through the C ABI.

What the engine selects on (csrc/engine_fft.inc.hpp dpp_le / degred_l, csrc/dpp.hpp, csrc/pss.hpp):

  * d_pp: dpp_tile_kernel<P, L, 8> / dpp_finish_kernel<P, L> for L = 1, 2, 4, 8 (8 / 4 / 2 / 1 chunks per thread; the
    unpack_accumulate bodies dot_k<4>, dot_k<8> and unpack_term over two or four groups of eight rows); tiles of 2048
    elements; dpp_carry_kernel with min(1024, max(64, roundup64(ntiles))) threads, ceil(ntiles / threads) tile totals per
    thread, two workgroups (scans | the one inversion)
  * deg_red: king_degred_coop_kernel for l = 2 with all 8 parties up to 2^16 chunks, king_degred_kernel<L> otherwise, in
    64-thread groups up to 2^16 chunks and 256-thread groups above; a party subset whose size is no multiple of the row
    group takes unpack_accumulate's row-at-a-time loop

Every output share is compared bit for bit.  Reference: oracle/cref.py CPss (the C restatement: one inverse() per element,
a serial prefix product, pack_vec, deg_red) in its threaded form, which tests/test_oracle_c.py pins on oracle/dist.py at
every packing factor; oracle/dist.py itself where a party is missing (the C side has no dropout).  Large inputs are raw
limb arrays below the modulus, i.e. Montgomery residues.  docs/degred_dpp_tests.md says which case reaches which shape.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import zksaas_amd as zk
from zksaas_amd import groth16 as zg
from zksaas_amd import synthetic
from zksaas_amd.api import deg_red_parties
from oracle import dist as od
from oracle import groth16 as og
from oracle.cref import CPss, lib as cref_lib
from oracle.field import Domain
from oracle.params import BN254, CURVES
from oracle.prng import rand_vec

from gpu_util import ctx, opp, up_parties, down_parties

ALL_CURVES = ["bn254", "bls12_381", "bls12_377"]
TILE = 2048                     # csrc/dpp.hpp DppGeom<DPP_E_LONG>::TILE
CARRY_THREADS = 1024            # DPP_CARRY_THREADS
KING_LIMIT = 1 << 16            # king_block / KING_COOP_MAX
REF_THREADS = 16                # threads of the C reference's king
THREE_TILES = 2 * TILE + 8 * 13


@functools.lru_cache(maxsize=None)
def cps(curve, l):
    return CPss(curve, l)


def _raw(count, seed):
    """any limbs below the modulus are a field element in Montgomery form: 2^252 < r on all three curves"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def _const(pp, value, count):
    return np.ascontiguousarray(np.tile(pp.fr.encode([value]), (count, 1)))


@contextlib.contextmanager
def _own_context(curve, l):
    """a context of the test's own: its scratch starts empty, and everything the test uploads is freed with it"""
    pp = zk.PackedSharingParams(curve, l)
    bufs = []

    def keep(buf):
        bufs.append(buf)
        return buf

    try:
        yield pp, keep
    finally:
        for b in bufs:
            b.free()
        pp.close()


@contextlib.contextmanager
def _shared_context(curve, l):
    """the suite's cached context of (curve, l) for the small cases; what the test uploads is freed at its end"""
    bufs = []

    def keep(buf):
        bufs.append(buf)
        return buf

    try:
        yield ctx(curve, l), keep
    finally:
        for b in bufs:
            b.free()


def _masks(pp, keep, ln, seed, which="both"):
    """DegRedMask.sample on the device, downloaded for the reference; `which` in none / in / out / both drops a side on
    BOTH paths.  Returns (device mask, in-mask limbs or None, out-mask limbs or None)."""
    if which == "none":
        return zk.DegRedMask.zero(), None, None
    mk = zk.DegRedMask.sample(pp, ln, seed)
    keep(mk.in_mask), keep(mk.out_mask)
    im = mk.in_mask.to_numpy().reshape(-1, 4).copy()
    om = mk.out_mask.to_numpy().reshape(-1, 4).copy()
    assert im.any() and om.any() and not np.array_equal(im, om)
    if which == "in":
        return zk.DegRedMask(mk.in_mask, None), im, None
    if which == "out":
        return zk.DegRedMask(None, mk.out_mask), None, om
    return mk, im, om


def _same(got, want, ln, what):
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d of %d shares differ, the first one party %d chunk %d" % (
        what, bad.size, got.shape[0], bad[0] // ln, bad[0] % ln)


def _ref_d_pp(cp, num, den, ln, im, om, seed):
    return cp.d_pp_arrays(num, den, ln, im, om, seed, threads=REF_THREADS)


def _ref_deg_red(cp, x, ln, im, om, seed):
    """zkref_deg_red on a copy, its king split over REF_THREADS threads"""
    want = x.copy()
    cref_lib().zkref_set_fast_king(1, REF_THREADS)
    try:
        cp.deg_red_arrays(want, ln, im, om, seed)
    finally:
        cref_lib().zkref_set_fast_king(0, 1)
    return want


def _d_pp_case(pp, keep, curve, l, num, den, ln, which, seed, what):
    """zk_d_pp of the share arrays num / den against the reference; returns the device result"""
    mask, im, om = _masks(pp, keep, ln, seed + 1, which)
    res = keep(zk.d_pp(pp, keep(zk.DeviceBuffer.from_numpy(pp, num)), keep(zk.DeviceBuffer.from_numpy(pp, den)), mask, ln,
                       seed=seed))
    _same(res.to_numpy(), _ref_d_pp(cps(curve, l), num, den, ln, im, om, seed), ln, what)
    return res


def carry_launch(ntiles):
    """(waves of a dpp_carry_kernel workgroup, tile totals per thread), from dpp_le's own formulas"""
    threads = min(CARRY_THREADS, max(64, (ntiles + 63) // 64 * 64))
    return threads // 64, (ntiles + threads - 1) // threads


def ntiles_of(m):
    return (m + TILE - 1) // TILE


# ================================================================================================ d_pp
EVERY_L = [("bn254", l, m) for l in (1, 2, 4, 8) for m in (l, TILE - l, TILE, TILE + l, THREE_TILES)]
BLS = [(c, l, THREE_TILES) for c in ("bls12_381", "bls12_377") for l in (1, 4, 8)]


@pytest.mark.parametrize("curve,l,m", EVERY_L + BLS, ids=["%s-l%d-m%d" % c for c in EVERY_L + BLS])
def test_d_pp_at_every_packing_factor(curve, l, m):
    """One chunk, a tile less one chunk, one tile exactly, a second tile holding one chunk and the padding ones, three
    tiles; sampled DegRedMask."""
    with _shared_context(curve, l) as (pp, keep):
        ln = m // l
        num, den = _raw(pp.n * ln, 100 + m), _raw(pp.n * ln, 200 + m)
        _d_pp_case(pp, keep, curve, l, num, den, ln, "both", 300 + l, "%s l=%d m=%d" % (curve, l, m))


CARRY_EXACT = ([("bn254", l, t, t * TILE - 6 * l) for l in (2, 8) for t in (64, 65, 129, 1000, 1024)]
               + [("bn254", 2, 1025, 1025 * TILE)])
CARRY_TELESCOPE = [(c, l, t, t * TILE - 6 * l) for c, l in (("bn254", 8), ("bls12_381", 2)) for t in (1500, 3073)]
_ID4 = ["%s-l%d-tiles%d-m%d" % c for c in CARRY_EXACT + CARRY_TELESCOPE]


def test_carry_cases_hold_every_launch_shape():
    """The case lists reach a carry workgroup of 1, 2, 3 and 16 waves and 1, 2 and 4 tile totals per thread; the partly
    filled multi-wave workgroups (65, 129, 1000 tiles), the ragged q = 2 (1025 tiles: threads 513 and up own nothing) and
    q = 4 with threads 769 and up idle (3073 tiles) among them -- so the lists cannot drift away from dpp_le."""
    shapes = {}
    for _, _, t, m in CARRY_EXACT + CARRY_TELESCOPE:
        assert ntiles_of(m) == t
        shapes.setdefault(carry_launch(t), []).append(t)
    waves, qs = {w for w, _ in shapes}, {q for _, q in shapes}
    assert {1, 2, 3, 16} <= waves and {1, 2, 4} <= qs
    assert carry_launch(64) == (1, 1) and carry_launch(65) == (2, 1) and carry_launch(129) == (3, 1)
    assert carry_launch(1000) == (16, 1) and carry_launch(1024) == (16, 1)
    assert carry_launch(1025) == (16, 2) and carry_launch(1500) == (16, 2) and carry_launch(3073) == (16, 4)
    # idle threads: a thread owns tiles [t q, t q + q); the first one past the end
    assert -(-1025 // 2) == 513 and -(-3073 // 4) == 769 and -(-1000 // 1) == 1000


@pytest.mark.parametrize("curve,l,ntiles,m", CARRY_EXACT, ids=_ID4[:len(CARRY_EXACT)])
def test_d_pp_carry_shapes_equal_c_oracle(curve, l, ntiles, m):
    with _own_context(curve, l) as (pp, keep):
        ln = m // l
        num, den = _raw(pp.n * ln, 400 + ntiles), _raw(pp.n * ln, 500 + ntiles)
        _d_pp_case(pp, keep, curve, l, num, den, ln, "both", 600 + l, "%s l=%d %d tiles" % (curve, l, ntiles))


@pytest.mark.parametrize("curve,l,ntiles,m", CARRY_TELESCOPE, ids=_ID4[len(CARRY_EXACT):])
def test_d_pp_carry_shapes_telescope(curve, l, ntiles, m):
    """num_i = x_(i+1), den_i = x_i  =>  prefix_i * x_0 = x_(i+1), all on the device (the property of
    test_gpu_fullsize.py::test_d_pp_telescopes_bls12_381_2_18) where a thread of the carry kernel owns 2 or 4 tile totals."""
    with _own_context(curve, l) as (pp, keep):
        eb, nl, ln = pp.fr.nbytes, pp.fr.nl, m // l
        x = keep(synthetic.rand_fr_device(pp, m + 1, 700 + ntiles))
        num_sh, den_sh = keep(pp.pack(x.view(eb), ln, 701)), keep(pp.pack(x, ln, 702))
        res = keep(zk.d_pp(pp, num_sh, den_sh, zk.DegRedMask.zero(), ln, seed=703))
        prod = keep(pp.unpack(res, ln))
        zk.api.vec_scale(pp, prod, pp.download_fr(x, 1)[0], m)
        got, want = prod.to_numpy()[: m * nl].reshape(m, nl), x.to_numpy()[nl:(m + 1) * nl].reshape(m, nl)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "%d of %d prefix products differ, the first at element %d (tile %d)" % (
            bad.size, m, bad[0], bad[0] // TILE)


WHICH = [(l, w) for l in (2, 4) for w in ("none", "in", "out", "both")]


@pytest.mark.parametrize("l,which", WHICH, ids=["bn254-l%d-m%d-%s" % (l, THREE_TILES, w) for l, w in WHICH])
def test_d_pp_with_either_mask_pointer_null(l, which):
    """bn254, m = 4200 (three tiles): the finish kernel adds unpack2 of the in-mask and the out-mask independently of
    each other; the reference gets None for the absent one."""
    with _shared_context("bn254", l) as (pp, keep):
        ln = THREE_TILES // l
        num, den = _raw(pp.n * ln, 800 + l), _raw(pp.n * ln, 810 + l)
        _d_pp_case(pp, keep, "bn254", l, num, den, ln, which, 820, "bn254 l=%d m=%d masks %s" % (l, THREE_TILES, which))


EDGES = ["num_r-1", "num_zero_at_0", "num_zero_end_of_tile_0", "num_zero_in_last_tile", "den_1", "den_r-1"]


EDGE_CASES = [(c, l, e) for c in ALL_CURVES for l in (1, 2, 8) for e in EDGES]


@pytest.mark.parametrize("curve,l,edge", EDGE_CASES, ids=["%s-l%d-m%d-%s" % (c, l, THREE_TILES, e) for c, l, e in EDGE_CASES])
def test_d_pp_edge_values(curve, l, edge):
    """m = 4200 (three tiles, the last one padded): numerator SHARES all r - 1, numerators with a zero (the prefix is zero
    from there on and the call succeeds), denominator shares all 1 and all r - 1."""
    m = THREE_TILES
    ln, r = m // l, CURVES[curve].r
    with _shared_context(curve, l) as (pp, keep):
        num, den = _raw(pp.n * ln, 900 + l), _raw(pp.n * ln, 910 + l)
        zero_at = None
        if edge == "num_r-1":
            num = _const(pp, r - 1, pp.n * ln)
        elif edge == "den_1":
            den = _const(pp, 1, pp.n * ln)
        elif edge == "den_r-1":
            den = _const(pp, r - 1, pp.n * ln)
        else:
            zero_at = {"num_zero_at_0": 0, "num_zero_end_of_tile_0": TILE - 1, "num_zero_in_last_tile": 2 * TILE + 37}[edge]
            sec = _raw(m, 920 + l)
            sec[zero_at] = 0
            num = keep(pp.pack(keep(zk.DeviceBuffer.from_numpy(pp, sec)), ln, seed=921)).to_numpy().reshape(-1, 4).copy()
        res = _d_pp_case(pp, keep, curve, l, num, den, ln, "both", 930, "%s l=%d m=%d %s" % (curve, l, m, edge))
        if zero_at is not None:
            prefix = keep(pp.unpack(res, ln)).to_numpy().reshape(m, 4)           # the masks cancel
            assert not prefix[zero_at:].any() and prefix[:zero_at].any(axis=1).all()


ZERO_TILES = 129
ZERO_AT = {"element_0": lambda m: 0, "last_element": lambda m: m - 1,
           "first_of_last_partial_tile": lambda m: (ZERO_TILES - 1) * TILE, "inside_tile_70": lambda m: 70 * TILE + 999}


@pytest.fixture(scope="module", params=[2, 8], ids=["bn254-l2-tiles129", "bn254-l8-tiles129"])
def zero_den(request):
    """129 tiles (three carry waves; tile 70's denominator total belongs to thread 121 of workgroup 1, its second wave):
    packed random secrets, the correct call's reference computed once for the positions that follow"""
    l = request.param
    m = ZERO_TILES * TILE - 6 * l
    with _own_context("bn254", l) as (pp, keep):
        ln = m // l
        assert carry_launch(ntiles_of(m)) == (3, 1) and (192 - 1 - 70) // 64 == 1
        num = _raw(pp.n * ln, 1000 + l)
        den_sec = _raw(m, 1010 + l)
        den = keep(pp.pack(keep(zk.DeviceBuffer.from_numpy(pp, den_sec)), ln, seed=1011)).to_numpy().reshape(-1, 4).copy()
        mask, im, om = _masks(pp, keep, ln, 1012)
        want = _ref_d_pp(cps("bn254", l), num, den, ln, im, om, 1013)
        yield dict(pp=pp, l=l, m=m, ln=ln, num=num, num_d=keep(zk.DeviceBuffer.from_numpy(pp, num)), den=den,
                   den_d=keep(zk.DeviceBuffer.from_numpy(pp, den)), den_sec=den_sec, mask=mask, want=want)


@pytest.mark.parametrize("where", list(ZERO_AT), ids=["zero_at_" + w for w in ZERO_AT])
def test_d_pp_zero_denominator_is_code_1_and_the_next_call_is_exact(zero_den, where):
    """dpp/mod.rs:55 inverse().unwrap(): the call fails with code 1 wherever the zero sits; the next, correct d_pp on the
    same context and stream equals the reference -- neither the error flag, nor the ready word, nor the inverse the failed
    call published is seen by it."""
    z = zero_den
    pp, m, ln = z["pp"], z["m"], z["ln"]
    at = ZERO_AT[where](m)
    assert 0 <= at < m and (where != "inside_tile_70" or at // TILE == 70)
    sec = z["den_sec"].copy()
    sec[at] = 0
    sec_d = zk.DeviceBuffer.from_numpy(pp, sec)
    bad_d = pp.pack(sec_d, ln, seed=1011)
    out = pp.alloc_fr(pp.n * ln)
    try:
        with pytest.raises(zk.ZkError) as e:
            zk.d_pp(pp, z["num_d"], bad_d, z["mask"], ln, seed=1013, out=out)
        assert e.value.code == 1
        if where == "inside_tile_70":                      # the reference refuses it as well (once: 2^18 inversions)
            with pytest.raises(ZeroDivisionError):
                _ref_d_pp(cps("bn254", z["l"]), z["num"], bad_d.to_numpy().reshape(-1, 4).copy(), ln, None, None, 1013)
        zk.d_pp(pp, z["num_d"], z["den_d"], z["mask"], ln, seed=1013, out=out)
        _same(out.to_numpy(), z["want"], ln, "d_pp after a zero denominator at %s" % where)
    finally:
        for b in (sec_d, bad_d, out):
            b.free()


def test_d_pp_sequence_of_sizes_on_one_context():
    """bn254 l = 2 on a fresh context: 129 tiles, one chunk, 65 tiles, 129 tiles again with other data -- the scratch
    grows, is reused at a smaller and at the same size, and no call sees an earlier call's 1 / D or tile totals."""
    l = 2
    with _own_context("bn254", l) as (pp, keep):
        for step, (m, seed) in enumerate(((129 * TILE - 6 * l, 1100), (l, 1101), (65 * TILE - 6 * l, 1102),
                                          (129 * TILE - 6 * l, 1103))):
            ln = m // l
            num, den = _raw(pp.n * ln, seed), _raw(pp.n * ln, seed + 50)
            _d_pp_case(pp, keep, "bn254", l, num, den, ln, "both", seed + 100, "step %d, m = %d" % (step, m))


# ================================================================================================ deg_red
def _deg_red_case(curve, l, nch, which="both", x=None, masks_np=None, seed=1200):
    """zk_deg_red in place on raw share limbs against the reference; a context of its own above the 2^16 boundary"""
    with (_own_context if nch > 4096 else _shared_context)(curve, l) as (pp, keep):
        x = _raw(pp.n * nch, seed + nch % 1000) if x is None else x
        if masks_np is None:
            mask, im, om = _masks(pp, keep, nch, seed + 1, which)
        else:
            im, om = masks_np
            mask = zk.DegRedMask(keep(zk.DeviceBuffer.from_numpy(pp, im)), keep(zk.DeviceBuffer.from_numpy(pp, om)))
        buf = keep(zk.DeviceBuffer.from_numpy(pp, x))
        zk.deg_red(pp, buf, mask, nch, seed=seed + 2)
        _same(buf.to_numpy(), _ref_deg_red(cps(curve, l), x, nch, im, om, seed + 2), nch,
              "%s l=%d nch=%d masks %s" % (curve, l, nch, which))


DEGRED_L = [("bn254", 1), ("bn254", 2), ("bn254", 4), ("bn254", 8), ("bls12_381", 1), ("bls12_381", 8), ("bls12_377", 1),
            ("bls12_377", 8)]


DEGRED_CASES = [(c, l, nch) for c, l in DEGRED_L for nch in (1, 7, 8, 9, 63, 64, 65, 331)]


@pytest.mark.parametrize("curve,l,nch", DEGRED_CASES, ids=["%s-l%d-nch%d" % c for c in DEGRED_CASES])
def test_deg_red_at_every_packing_factor(curve, l, nch):
    """around the cooperative kernel's eight chunks per workgroup and the 64-thread group; 331: six groups, the last ragged"""
    _deg_red_case(curve, l, nch)


BOUNDARY = [(2, KING_LIMIT - 1), (2, KING_LIMIT), (2, KING_LIMIT + 1), (1, KING_LIMIT), (1, KING_LIMIT + 1),
            (4, KING_LIMIT), (4, KING_LIMIT + 1), (8, KING_LIMIT + 1)]


@pytest.mark.parametrize("l,nch", BOUNDARY, ids=["bn254-l%d-nch%d" % c for c in BOUNDARY])
def test_deg_red_on_both_sides_of_2_16_chunks(l, nch):
    """bn254.  l = 2: the cooperative kernel's last grid (65 535, 65 536), then king_degred_kernel<2> in 256-thread groups;
    l = 1, 4: the last launch in 64-thread groups and the first in 256-thread ones; l = 8 above."""
    _deg_red_case("bn254", l, nch)


@pytest.mark.parametrize("l", [1, 2, 4, 8], ids=["bn254-l%d-nch70" % l for l in (1, 2, 4, 8)])
def test_deg_red_out_of_place_with_all_parties(l):
    """bn254, nch = 70: zk_deg_red_parties over parties 0 .. n - 1 with out != x gives the in-place shares and leaves x alone"""
    pp, nch = ctx("bn254", l), 70
    x = _raw(pp.n * nch, 1300 + l)
    mk = zk.DegRedMask.sample(pp, nch, 1301)
    src, inplace = zk.DeviceBuffer.from_numpy(pp, x), zk.DeviceBuffer.from_numpy(pp, x)
    try:
        out = deg_red_parties(pp, src, list(range(pp.n)), mk, nch, seed=1302)
        zk.deg_red(pp, inplace, mk, nch, seed=1302)
        assert np.array_equal(src.to_numpy().reshape(-1, 4), x)
        _same(out.to_numpy(), inplace.to_numpy(), nch, "out of place, l=%d" % l)
        _same(out.to_numpy(), _ref_deg_red(cps("bn254", l), x, nch, mk.in_mask.to_numpy().reshape(-1, 4).copy(),
                                           mk.out_mask.to_numpy().reshape(-1, 4).copy(), 1302), nch, "reference, l=%d" % l)
    finally:
        for b in (src, inplace, out, mk.in_mask, mk.out_mask):
            b.free()


@functools.lru_cache(maxsize=None)
def _products(l, nch):
    """bn254: secrets, the squares of their shares (degree 2 (l + t - 1)) and a sampled oracle mask, built once"""
    o = opp("bn254", l)
    secrets = rand_vec(1400 + l, nch * l, o.p)
    shares = od.transpose(od.pack_vec(secrets, o, 1401))
    mul = [[v * v % o.p for v in row] for row in shares]
    return secrets, mul, od.DegRedMask.sample(o, 1, nch, 1402)


DROPOUT = ([(2, d, w) for d in range(8) for w in ("none", "both")]
           + [(l, d, w) for l in (1, 4, 8) for d in (0, 2 * l, 4 * l - 1) for w in ("none", "both")]
           + [(2, 5, "in"), (2, 5, "out"), (8, 0, "in"), (8, 0, "out")])


DROPOUT_CASES = [(l, d, w, nch) for l, d, w in DROPOUT for nch in (13, 70)]


@pytest.mark.parametrize("l,drop,which,nch", DROPOUT_CASES,
                         ids=["bn254-l%d-nch%d-without%d-masks_%s" % (l, nch, d, w) for l, d, w, nch in DROPOUT_CASES])
def test_deg_red_with_a_missing_party(l, drop, which, nch):
    """bn254: the king got n - 1 rows (ser_net.rs:57-94 -> lagrange_unpack).  x and the in-mask are [n - 1][nch] in LISTED
    order, the out-mask and the result [n][nch].  Shares bit for bit against oracle/dist.py deg_red(parties=); with both
    masks or none, unpack gives the products.  70 chunks: two 64-thread groups."""
    pp, o = ctx("bn254", l), opp("bn254", l)
    secrets, mul, masks = _products(l, nch)
    zero = [0] * nch
    omasks = [od.DegRedMask(k.in_mask if which in ("in", "both") else zero, k.out_mask if which in ("out", "both") else zero)
              for k in masks]
    parties = [i for i in range(o.n) if i != drop]
    want = od.deg_red(mul, omasks, o, seed=1403, parties=parties)
    im = up_parties(pp, [masks[i].in_mask for i in parties]) if which in ("in", "both") else None
    om = up_parties(pp, [k.out_mask for k in masks]) if which in ("out", "both") else None
    out = deg_red_parties(pp, up_parties(pp, [mul[i] for i in parties]), parties, zk.DegRedMask(im, om), nch, seed=1403)
    assert down_parties(pp, out, pp.n, nch) == want
    if which in ("none", "both"):
        assert pp.download_fr(pp.unpack(out, nch)) == [v * v % o.p for v in secrets]


@pytest.mark.parametrize("l", [1, 2, 4, 8], ids=["bn254-l%d-nch13" % l for l in (1, 2, 4, 8)])
def test_deg_red_with_two_missing_parties_is_protocol_error(l):
    """products have degree 2 (l + t - 1) = n - 2: n - 1 rows are needed (as unpack2 in
    test_gpu_pss.py::test_not_enough_shares_is_protocol_error)"""
    pp, nch = ctx("bn254", l), 13
    parties = list(range(pp.n - 2))
    with pytest.raises(zk.ZkError) as e:
        deg_red_parties(pp, pp.alloc_fr(len(parties) * nch), parties, zk.DegRedMask.zero(), nch, seed=1)
    assert e.value.code == 2


@pytest.mark.parametrize("l,which", WHICH, ids=["bn254-l%d-nch331-%s" % c for c in WHICH])
def test_deg_red_with_either_mask_pointer_null(l, which):
    """bn254, nch = 331: king_degred_coop_kernel (l = 2) and king_degred_kernel<4>"""
    _deg_red_case("bn254", l, 331, which, seed=1500)


DEGRED_EDGES = [(c, l, v) for c in ALL_CURVES for l in (1, 2, 8) for v in ("r-1", "zero")]


@pytest.mark.parametrize("curve,l,value", DEGRED_EDGES, ids=["%s-l%d-nch65-%s" % c for c in DEGRED_EDGES])
def test_deg_red_edge_values(curve, l, value):
    """nch = 65.  Shares all r - 1 under masks all r - 1 (every row the king unpacks is r - 2, the out-mask adds r - 1 to
    every share), and shares all zero: the one-reduction dot products of unpack_accumulate and pack_row at their largest
    operands."""
    pp, nch, r = ctx(curve, l), 65, CURVES[curve].r
    if value == "r-1":
        x = _const(pp, r - 1, pp.n * nch)
        _deg_red_case(curve, l, nch, "both", x=x, masks_np=(x.copy(), x.copy()), seed=1600)
    else:
        _deg_red_case(curve, l, nch, "none", x=np.zeros((pp.n * nch, 4), dtype=np.uint64), seed=1610)


def test_deg_red_edge_values_in_the_256_thread_class_at_l_2():
    """bn254, 65 537 chunks of r - 1 under masks of r - 1: king_degred_kernel<2>'s eight-row dot product (dot_k<8>), which
    the cooperative kernel keeps every shorter l = 2 vector away from"""
    nch = KING_LIMIT + 1
    x = _const(ctx("bn254", 2), BN254.r - 1, 8 * nch)
    _deg_red_case("bn254", 2, nch, "both", x=x, masks_np=(x.copy(), x.copy()), seed=1620)


@pytest.mark.parametrize("l", [1, 4, 8], ids=["bn254-l%d-m64" % l for l in (1, 4, 8)])
def test_circom_h_forms_a_b_minus_c_at_the_load(l):
    """bn254, m = 64, all six FFT masks and the DegRedMask: zk_circom_h's last step is king_degred_kernel<1|4|8> with
    mul_b / sub_c (a * b - c formed at the load, ext_wit.rs:173-177).  Shares equal oracle/groth16.py circom_h; unpack2
    gives circom_ref.  (l = 2, the cooperative kernel: tests/test_gpu_groth16.py.)"""
    m, log_m, P = 64, 6, BN254.r
    pp, o = ctx("bn254", l), opp("bn254", l)
    dom = Domain(BN254, m)
    a = list(range(m))
    c = [v * v % P for v in a]
    qs = og.QAP(0, 0, a, a, c, dom).pss(o, 3)
    w2m = Domain(BN254, 2 * m).element(1)
    fm = ([od.FftMask.sample(True, w2m, dom.group_gen_inv, m, o, 40 + k) for k in range(3)]
          + [od.FftMask.sample(False, 1, dom.group_gen, m, o, 50 + k) for k in range(3)])
    dm = od.DegRedMask.sample(o, 1, m // l, 60)
    want = og.circom_h(qs, fm, dm, o, dom, seed=4)
    bufs = [up_parties(pp, [qs[i][k] for i in range(o.n)]) for k in range(3)]
    keep = []
    mk = zg.Masks()
    for k in range(6):
        bi, bo = up_parties(pp, [v.in_mask for v in fm[k]]), up_parties(pp, [v.out_mask for v in fm[k]])
        keep += [bi, bo]
        mk.fft_in[k], mk.fft_out[k] = bi.ptr, bo.ptr
    di, do = up_parties(pp, [v.in_mask for v in dm]), up_parties(pp, [v.out_mask for v in dm])
    mk.degred_in, mk.degred_out = di.ptr, do.ptr
    h = pp.alloc_fr(o.n * (m // l))
    pp._check(pp.lib.zk_circom_h(pp.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, log_m, C.byref(mk), 4, h.ptr, None))
    assert down_parties(pp, h, o.n, m // l) == want
    assert pp.download_fr(pp.unpack2(h, m // l)) == og.circom_ref(a, a, c, dom)
