"""The pass plan of fft1 restated in plain Python (no GPU, no C++): which stages each ntt_pass_kernel launch covers at a
transform size, which global indices one workgroup's tile holds, and where the shapes change.  tests/test_ntt_plan.py
compares it with csrc/ntt.hpp's make_ntt_plan line by line; tests/test_gpu_ntt_sizes.py takes its size grids and the
positions worth sampling from here.  (The same role tests/msm_digits.py has for the MSM.)"""
import numpy as np

TILE_BITS_SMALL, TILE_BITS_LARGE, SMALL_MAX_LOG_N = 8, 11, 14
MAX_PASSES = 4
TWO_ADICITY = {"bn254": 28, "bls12_381": 32, "bls12_377": 47}


def tile_bits(log_n):
    """Tile of the engine at this size; None below 2^8, where one launch per stage works straight from memory."""
    if log_n < TILE_BITS_SMALL:
        return None
    return TILE_BITS_SMALL if log_n <= SMALL_MAX_LOG_N else TILE_BITS_LARGE


def plan(log_n, tb=None):
    """[(s0, s1, cbits)] per pass: the pass runs stages s0+1 .. s1 on tiles of 2^cbits adjacent columns.

    Stated from the rules, not from the code: the first pass may take tb stages, a later one tb - 2; use as few passes
    as that allows; share the stages as evenly as possible, earlier passes taking the odd ones; what a later pass
    cannot hold goes to the first; a tile takes as many columns as fit beside its 2^(s1-s0) rows, but no more than the
    2^s0 there are."""
    tb = tile_bits(log_n) if tb is None else tb
    if log_n <= tb:
        return [(0, log_n, 0)]
    later = tb - 2
    npass = 1 + -(-(log_n - tb) // later)
    if npass > MAX_PASSES:
        raise ValueError("2^%d needs %d passes on 2^%d-element tiles" % (log_n, npass, tb))
    share = [log_n // npass + (1 if i < log_n % npass else 0) for i in range(npass)]
    overflow = sum(max(0, s - later) for s in share[1:])
    share = [share[0] + overflow] + [min(s, later) for s in share[1:]]
    out, done = [], 0
    for stages in share:
        out.append((done, done + stages, min(tb - stages, done)))
        done += stages
    return out


def tile_indices(log_n, tb, s0, s1, cbits):
    """int64 [tiles][2^tb]: the global index that slot x of workgroup blockIdx.x loads and stores, by the kernel's own
    formula (h0, c0 from blockIdx.x; c, r, hb from the slot)."""
    rbits = s1 - s0
    hbbits = tb - rbits - cbits
    assert hbbits >= 0
    bx = np.arange(1 << (log_n - tb), dtype=np.int64)[:, None]
    x = np.arange(1 << tb, dtype=np.int64)[None, :]
    if hbbits > 0 or cbits == s0:
        h0, c0 = bx << hbbits, 0 * bx
    else:
        per_h = 1 << (s0 - cbits)
        h0, c0 = bx // per_h, (bx % per_h) << cbits
    c = x & ((1 << cbits) - 1)
    r = (x >> cbits) & ((1 << rbits) - 1)
    hb = x >> (cbits + rbits)
    return ((h0 + hb) << s1) + (r << s0) + c0 + c


def pass_shape(log_n, tb, s0, s1, cbits):
    """The branches of ntt_pass_kernel one pass takes, as a dict of small facts (docs/ntt_size_tests.md's table)."""
    rbits = s1 - s0
    hbbits = tb - rbits - cbits
    tws = 2 if (tb >= 10 and rbits >= 4) else 0
    return {"odd": rbits & 1, "hb": hbbits > 0, "rows": hbbits > 0 or cbits == s0, "tws": tws,
            "hbm_twiddles": tws == 2, "lds_twiddles": (((1 << rbits) // 2) >> tws) + 1}


# ---- size grids of tests/test_gpu_ntt_sizes.py
FFT1_FULL = ([("bn254", l, k) for l in (1, 2, 4, 8) for k in range(0, 21)] +
             [(c, 2, k) for c in ("bls12_381", "bls12_377") for k in range(0, 21)] +
             [("bn254", 2, k) for k in (21, 22, 23, 24)])
FFT1_SAMPLED = [("bn254", 2, k) for k in (25, 26, 27)]


def sample_positions(log_n, count=64, seed=2718):
    """Outputs of a 2^log_n transform worth evaluating one by one: a fixed-seed sample, the first and last index of the
    first and last tile, and both neighbours of every pass's row boundary (k = 2^s0 - 1, 2^s0)."""
    n = 1 << log_n
    tb = tile_bits(log_n) or 0
    rng = np.random.default_rng(seed + log_n)
    ks = set(int(v) for v in rng.integers(0, n, size=count))
    while len(ks) < min(count, n):
        ks.add(int(rng.integers(0, n)))
    tile = min(n, 1 << tb)
    ks |= {0, tile - 1, n - tile, n - 1}
    if tb:
        for s0, _s1, _cb in plan(log_n, tb):
            ks |= {(1 << s0) - 1, min(n - 1, 1 << s0)}
    return sorted(ks)


def king_class(lc):
    """The three launch shapes of king_fft2_kernel by Lc = m / l chunks."""
    return "below64" if lc < 64 else ("wave" if lc <= (1 << 16) else "block")
