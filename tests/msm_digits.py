"""Window geometry, signed-digit recoding and scalar construction of the Pippenger MSM, restated in plain Python
integers from the comments in csrc/msm_plan.hpp (MsmWindows) / csrc/msm.hpp (nothing is imported from the library): the tests
choose the digits the sort kernels see instead of hoping that random scalars reach them.

A launch spreads T = BITS + 1 bits (room for the signed-digit carry) evenly over nwin = ceil(T / c_req) windows:
`wide` windows of c = ceil(T / nwin) bits, then nwin - wide windows of c - 1.  Digits lie in (-half, +half] with
half = 2^(cw - 1): +half stays positive (magnitude half is bucket k = half, the largest), half + 1 becomes
-(half - 1) with a carry into the next window.  A fixed-base table uses the same split of its own width; its digits
are the same, but all windows fall into ONE set of B = 2^(c-1) buckets.
"""
from collections import namedtuple

import numpy as np

Geometry = namedtuple("Geometry", "bits T c_req nwin c wide B widths starts table")


def geometry(r, c_req, table=False):
    """The window layout of a launch over the scalar field of order r at requested width c_req."""
    bits = r.bit_length()
    T = bits + 1
    nwin = (T + c_req - 1) // c_req
    c = (T + nwin - 1) // nwin
    wide = T - nwin * (c - 1)
    assert 1 <= wide <= nwin
    widths = tuple(c if w < wide else c - 1 for w in range(nwin))
    starts = tuple(sum(widths[:w]) for w in range(nwin))
    assert starts[-1] + widths[-1] == T
    return Geometry(bits, T, c_req, nwin, c, wide, 1 << (c - 1), widths, starts, bool(table))


def half(geo, w):
    return 1 << (geo.widths[w] - 1)


def recode(s, geo):
    """The signed digits of s, lowest window first (the walk of msm_for_each_digit / msm_next_digit)."""
    assert 0 <= s < (1 << geo.bits)
    digits, carry = [], 0
    for cw in geo.widths:
        d = (s & ((1 << cw) - 1)) + carry
        s >>= cw
        if d > (1 << (cw - 1)):
            d -= 1 << cw
            carry = 1
        else:
            carry = 0
        digits.append(d)
    assert s == 0 and carry == 0           # T = BITS + 1 bits always hold the last carry
    return digits


def compose(digits, geo):
    return sum(d << st for d, st in zip(digits, geo.starts))


def nonzero_digits(s, geo):
    """Mixed additions scalar s costs on a non-identity base: what zk_msm_stats must count for it."""
    return sum(1 for d in recode(s, geo) if d)


def top_limit(r, geo):
    """Digits of the top window must stay below this for the scalar to stay below r."""
    return r >> geo.starts[-1]


def engineered_digits(i, r, geo):
    """The chosen digits of engineered scalar i (0 <= i < 2B): k = i // 2 + 1, base sign + for even i and - for odd; in
    window w the magnitude is ((k - 1 + w) mod half_w) + 1 and the sign alternates with w; -half_w is entered as
    +half_w.  The top digit is positive, non-zero and below r >> start_top, so that 0 < s < r.  Where r >> start_top is
    1 (the top window holds r's leading bit alone) the top digit is 1 above a negative digit and 0 above a positive one
    (0 < s < 2^start_top <= r either way, and the window below keeps both signs); where it is 0 (the top window only
    ever takes a carry) the top digit is 0 and the digit below it is made positive: see free_windows."""
    k = i // 2 + 1
    top = geo.nwin - 1
    lim = top_limit(r, geo)
    ds = []
    for w in range(geo.nwin):
        h = half(geo, w)
        m = (k - 1 + w) % h + 1
        neg = (i + w) & 1
        if w == top:
            d = (k - 1 + w) % (lim - 1) + 1 if lim > 1 else int(lim == 1 and ds[-1] < 0)
        elif w == top - 1 and lim == 0:
            d = m
        else:
            d = m if (not neg or m == h) else -m
        ds.append(d)
    return ds


def free_windows(r, geo):
    """Windows whose digit the construction chooses freely, i.e. that receive every digit of (-half, +half] \\ {0}: all
    below the top one -- or below the one under it where r >> start_top == 0, because that window then holds r's
    leading bits and the top one only its carry (BN254 at c_req = 2)."""
    return geo.nwin - 1 if top_limit(r, geo) >= 1 else geo.nwin - 2


def engineered(r, geo, indices=None):
    """Scalars built FROM the digits of engineered_digits: s = sum_w d_w 2^(start_w).  The digit range of a window is a
    complete residue system mod 2^cw, so the recoding of s is exactly the chosen digits."""
    idx = range(2 * geo.B) if indices is None else indices
    return [compose(engineered_digits(i, r, geo), geo) for i in idx]


def half_digit_scalar(r, geo):
    """+half in every window at once (below the top one, whose digit keeps the scalar below r)."""
    ds = [half(geo, w) for w in range(geo.nwin)]
    lim = top_limit(r, geo)
    ds[-1] = min(lim - 1, ds[-1]) if lim > 1 else 0
    return compose(ds, geo)


def edge_scalars(r, geo):
    """0, 1, 2, r-1, r-2, (r-1)/2, (r+1)/2; 2^k - 1, 2^k, 2^k + 1 for every k < T below r (carry chains of every length,
    starting and ending in every window); per window the scalar whose only non-zero digit is +half_w and the one that
    is half_w + 1 there (-(half_w - 1) and a carry); +half in every window."""
    out = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2]
    for k in range(geo.T):
        for v in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if v < r:
                out.append(v)
    for w in range(geo.nwin):
        for v in (half(geo, w) << geo.starts[w], (half(geo, w) + 1) << geo.starts[w]):
            if v < r:
                out.append(v)
    out.append(half_digit_scalar(r, geo))
    return out


def table_indices(geo, count=1 << 16):
    """With a table above 16 bits the tests run `count` of the 2B engineered scalars: those whose magnitude is B, B - 1,
    1 or 2 in some window (both signs: i = 2 (k - 1) and 2 (k - 1) + 1), then an even stride over the rest."""
    if 2 * geo.B <= count:
        return list(range(2 * geo.B))
    want = set()
    for w in range(geo.nwin):
        h = half(geo, w)
        for m in (h, h - 1, 1, 2):
            # magnitude ((k - 1 + w) mod h) + 1 == m  <=>  k - 1 == m - 1 - w (mod h); every such k in [1, B]
            k0 = (m - 1 - w) % h
            for km1 in range(k0, geo.B, h):
                want.update((2 * km1, 2 * km1 + 1))
    n, step, phase = 2 * geo.B, 2 * geo.B // count, 0
    while len(want) < count:                           # evenly spread passes until the count is reached exactly
        for i in range(phase, n, step):
            want.add(i)
            if len(want) == count:
                break
        phase += 1
    return sorted(want)


# ------------------------------------------------------------------------------------------------- numpy forms
def engineered_digit_array(r, geo, indices=None):
    """engineered_digits for many i at once: int64 array [len(indices)][nwin]."""
    i = np.arange(2 * geo.B, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64)
    km1 = i // 2
    top = geo.nwin - 1
    lim = top_limit(r, geo)
    out = np.empty((i.size, geo.nwin), dtype=np.int64)
    for w in range(geo.nwin):
        h = half(geo, w)
        m = (km1 + w) % h + 1
        neg = ((i + w) & 1).astype(bool)
        if w == top:
            d = (km1 + w) % (lim - 1) + 1 if lim > 1 else ((out[:, w - 1] < 0) & (lim == 1)).astype(np.int64)
        elif w == top - 1 and lim == 0:
            d = m
        else:
            d = np.where(neg & (m != h), -m, m)
        out[:, w] = d
    return out


def digits_to_limbs(digits, geo, nl):
    """Canonical little-endian 64-bit limbs [n][nl] of s = sum_w d_w 2^(start_w) for an int64 digit array [n][nwin]
    whose every row composes to a non-negative value: the signed digits become the unsigned window values with a
    borrow that runs upwards, and the windows are disjoint bit fields."""
    n = digits.shape[0]
    limbs = np.zeros((n, nl), dtype=np.uint64)
    borrow = np.zeros(n, dtype=np.int64)
    for w in range(geo.nwin):
        cw, st = geo.widths[w], geo.starts[w]
        v = digits[:, w] - borrow
        borrow = (v < 0).astype(np.int64)
        u = (v + (borrow << cw)).astype(np.uint64)
        li, sh = st // 64, st % 64
        limbs[:, li] |= u << np.uint64(sh)
        if sh + cw > 64:
            limbs[:, li + 1] |= u >> np.uint64(64 - sh)
    assert not borrow.any(), "a digit row composes to a negative value"
    return limbs


def ints_to_limbs(vals, nl):
    return np.frombuffer(b"".join(int(v).to_bytes(8 * nl, "little") for v in vals), dtype=np.uint64).reshape(-1, nl).copy()


def limbs_to_ints(limbs):
    nl = limbs.shape[1]
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 8 * nl], "little") for i in range(0, len(raw), 8 * nl)]


def montgomery_limbs(limbs, r):
    """Canonical limbs -> Montgomery limbs (x R mod r, R = 2^(64 nl)), the form the library keeps scalars in."""
    nl = limbs.shape[1]
    R = (1 << (64 * nl)) % r
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    nb = 8 * nl
    out = b"".join((int.from_bytes(raw[i:i + nb], "little") * R % r).to_bytes(nb, "little") for i in range(0, len(raw), nb))
    return np.frombuffer(out, dtype=np.uint64).reshape(-1, nl)


def aggregate(limbs, cls, ncls, live, r):
    """agg[j] = sum of the scalars (canonical limbs [n][nl]) with live[i] and cls[i] == j, mod r; exact: 32-bit half
    limbs are summed in 64-bit words (n < 2^31 values below 2^32 cannot overflow)."""
    assert limbs.shape[0] < (1 << 31)
    nl = limbs.shape[1]
    agg = []
    for j in range(ncls):
        sel = limbs[live & (cls == j)]
        lo = (sel & np.uint64(0xFFFFFFFF)).sum(axis=0, dtype=np.uint64)
        hi = (sel >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
        agg.append(sum((int(lo[k]) + (int(hi[k]) << 32)) << (64 * k) for k in range(nl)) % r)
    return agg
