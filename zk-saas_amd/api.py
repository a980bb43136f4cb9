"""Host-side mirror of the reference interface (same names and argument meaning) over the C ABI.

reference                                           here
---------                                           ----
secret_sharing::pss::PackedSharingParams::new(l)     PackedSharingParams(curve, l)  (owns a zk_ctx)
  .pack / .det_pack / .unpack / .unpack2              same names, batched over chunks
  .lagrange_unpack(shares, parties)                   same
dist_primitives::dfft::{d_fft, d_ifft, FftMask}       d_fft, d_ifft, FftMask.sample / FftMask.zero
dist_primitives::dmsm::{d_msm, MsmMask}               d_msm, MsmMask.zero
dist_primitives::utils::deg_red::{deg_red, DegRedMask} deg_red, DegRedMask.sample / .zero
dist_primitives::dpp::d_pp                            d_pp

The reference runs n parties as tasks that meet at a king; here the n parties' share vectors live in ONE
device buffer [n][m/l] and each call performs the whole round (clients + king) on the GPU.
Errors raise ZkError (MpcNetError mirror).
"""
import ctypes as C

import numpy as np

from . import fields
from ._lib import ZkError, load

ZK_G1, ZK_G2 = 1, 2


class DeviceBuffer:
    """A hipMalloc'ed buffer owned through the C ABI (zk_malloc / zk_free)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx._check(ctx.lib.zk_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, arr.nbytes)
        if arr.nbytes:
            ctx._check(ctx.lib.zk_memcpy_h2d(ctx.h, b.ptr, arr.ctypes.data, arr.nbytes, None))
        return b

    def to_numpy(self, dtype=np.uint64, shape=None):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if self.nbytes:
            self.ctx._check(self.ctx.lib.zk_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes, None))
        return out.reshape(shape) if shape is not None else out

    def view(self, offset_bytes, nbytes=None):
        """A non-owning window into this buffer (keeps the parent alive)."""
        v = DeviceBuffer.__new__(DeviceBuffer)
        v.ctx, v.parent, v.owner = self.ctx, self, False
        v.nbytes = self.nbytes - offset_bytes if nbytes is None else int(nbytes)
        if offset_bytes < 0 or v.nbytes < 0 or offset_bytes + v.nbytes > self.nbytes:
            raise ValueError("view outside the buffer")
        v.ptr = self.ptr + offset_bytes
        return v

    def free(self):
        if not getattr(self, "owner", True):
            self.ptr = None
            return
        if self.ptr:
            self.ctx.lib.zk_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):       # torch tensor on the GPU
        return x.data_ptr()
    return int(x)


# Options every context created by THIS process gets right after zk_ctx_create (zk_ctx_set_option): the test suite puts
# {"rng_replay": 1} here (tests/conftest.py; shares are compared bit for bit with the oracle).  Nothing reads the
# environment: a deployment cannot end up on the replayable share randomness by inheriting a variable.
DEFAULT_OPTIONS = {}


class Context:
    """zk_ctx: PackedSharingParams + cached tables on one device."""

    def __init__(self, curve="bn254", l=2, device=0):
        self.lib = load()
        self.curve = curve
        self.h = C.c_void_p()
        rc = self.lib.zk_ctx_create(fields.CURVE_IDS[curve], l, device, C.byref(self.h))
        if rc != 0:
            msg = self.lib.zk_last_error(self.h, None).decode() if self.h else "zk_ctx_create failed (no GPU?)"
            raise ZkError(rc, msg)
        self.l = self.lib.zk_ctx_l(self.h)
        self.n = self.lib.zk_ctx_n(self.h)
        self.t = self.l
        self.fr = fields.MontCodec(fields.FR[curve])
        self.fq = fields.MontCodec(fields.FQ[curve])
        for name, value in DEFAULT_OPTIONS.items():
            self.set_option(name, value)

    def _check(self, rc):
        if rc != 0:
            party = C.c_int(-1)
            msg = self.lib.zk_last_error(self.h, C.byref(party)).decode()
            raise ZkError(rc, msg, party.value)

    def close(self):
        if self.h:
            self.lib.zk_ctx_destroy(self.h)
            self.h = None

    def set_option(self, name, value):
        """zk_ctx_set_option: context tunables ("msm_bigsort_min")."""
        self._check(self.lib.zk_ctx_set_option(self.h, name.encode(), int(value)))

    # --- marshalling helpers ---------------------------------------------------------------------
    def upload_fr(self, vals):
        return DeviceBuffer.from_numpy(self, self.fr.encode(vals))

    def upload_u32(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        if arr.size == 0:
            arr = np.zeros(1, dtype=np.uint32)
        return DeviceBuffer.from_numpy(self, arr)

    def download_fr(self, buf, count=None):
        arr = buf.to_numpy()
        if count is not None:
            arr = arr[: count * self.fr.nl]
        return self.fr.decode(arr)

    def alloc_fr(self, count):
        return DeviceBuffer(self, count * self.fr.nbytes)

    def sync(self, stream=None):
        self._check(self.lib.zk_stream_sync(self.h, stream))


class PackedSharingParams(Context):
    """secret-sharing/src/pss.rs:19-66."""

    def pack(self, secrets_d, nchunks, seed, order=0, out=None, stream=None):
        out = out or self.alloc_fr(self.n * nchunks)
        self._check(self.lib.zk_pss_pack(self.h, _ptr(secrets_d), nchunks, order, seed, _ptr(out), stream))
        return out

    def det_pack(self, secrets_d, nchunks, order=0, out=None, stream=None):
        out = out or self.alloc_fr(self.n * nchunks)
        self._check(self.lib.zk_pss_det_pack(self.h, _ptr(secrets_d), nchunks, order, _ptr(out), stream))
        return out

    def unpack(self, shares_d, nchunks, out=None, stream=None):
        out = out or self.alloc_fr(self.l * nchunks)
        self._check(self.lib.zk_pss_unpack(self.h, _ptr(shares_d), nchunks, _ptr(out), stream))
        return out

    def unpack2(self, shares_d, nchunks, parties=None, out=None, stream=None):
        out = out or self.alloc_fr(self.l * nchunks)
        if parties is None:
            arr, np_ = None, self.n
        else:
            arr = (C.c_uint32 * len(parties))(*parties)
            np_ = len(parties)
        self._check(self.lib.zk_pss_unpack2(self.h, _ptr(shares_d), arr, np_, nchunks, _ptr(out), stream))
        return out

    def unpack_robust(self, shares_d, nchunks, dimension=None, want_message=False, stream=None, parties=None):
        """zk_pss_unpack_robust: the error-correcting unpack of all n parties' shares [n][nchunks] (gao.rs decode_to_message
        per chunk, with a verdict instead of a panic).  dimension: 2l (packed shares, the default) up to 4l - 1 (their
        products).  With `parties` (ascending ids) shares_d is [len(parties)][nchunks], the other parties are absent and the
        call is zk_pss_unpack_robust_parties: wrong shares among the listed are corrected up to (len(parties) - dimension) // 2
        per chunk, errpos and summary stay indexed by party id.  Returns a RobustUnpack; nothing is synchronised until its
        numbers are read."""
        k = 2 * self.l if dimension is None else int(dimension)
        r = RobustUnpack(self, nchunks, k, None if parties is None else list(parties))
        r.secrets = self.alloc_fr(self.l * nchunks)
        r.status = DeviceBuffer(self, nchunks)
        r.errpos = DeviceBuffer(self, 4 * nchunks)
        r.summary_d = DeviceBuffer(self, 8 * (3 + self.n))
        r.message = self.alloc_fr(k * nchunks) if want_message and k > 0 else None
        if parties is None:
            self._check(self.lib.zk_pss_unpack_robust(self.h, _ptr(shares_d), nchunks, k, _ptr(r.secrets), _ptr(r.message),
                                                      _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        else:
            arr = (C.c_uint32 * len(r.parties))(*r.parties)
            self._check(self.lib.zk_pss_unpack_robust_parties(self.h, _ptr(shares_d), arr, len(r.parties), nchunks, k,
                                                              _ptr(r.secrets), _ptr(r.message), _ptr(r.status),
                                                              _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r

    def _report(self, nchunks, dimension, parties=None, words=1):
        """the verdict buffers of a repair or of a checked king round: a RobustUnpack without secrets and message.  words:
        the number of words checked (d_pp: 2) -- nchunks counts all their chunks, summary_d holds one summary per word"""
        r = RobustUnpack(self, nchunks, dimension, None if parties is None else list(parties))
        r.status = DeviceBuffer(self, nchunks)
        r.errpos = DeviceBuffer(self, 4 * nchunks)
        r.summary_d = DeviceBuffer(self, 8 * (3 + self.n) * words)
        return r

    def repair(self, shares_d, nchunks, dimension=None, stream=None, parties=None):
        """zk_pss_repair: unpack_robust's verdicts written back into shares_d [n][nchunks], in place: in a corrected chunk the
        share of every party named in errpos becomes the decoded polynomial's value, every other element keeps its bytes.
        With `parties` (ascending ids) shares_d is [len(parties)][nchunks], the other parties are absent and the call is
        zk_pss_repair_parties: the verdicts are unpack_robust's with that list, a named party's share is written at its row.
        Returns a RobustUnpack with status, errpos and summary (no secrets, no message); `out` is shares_d."""
        k = 2 * self.l if dimension is None else int(dimension)
        r = self._report(nchunks, k, parties)
        r.out = shares_d
        if parties is None:
            self._check(self.lib.zk_pss_repair(self.h, _ptr(shares_d), nchunks, k, _ptr(r.status), _ptr(r.errpos),
                                               _ptr(r.summary_d), stream))
        else:
            arr = (C.c_uint32 * len(r.parties))(*r.parties)
            self._check(self.lib.zk_pss_repair_parties(self.h, _ptr(shares_d), arr, len(r.parties), nchunks, k, _ptr(r.status),
                                                       _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r

    def repair_batch(self, shares_d, nitems, nchunks, dimension=None, item_stride=None, stream=None, parties=None):
        """zk_pss_repair_batch: repair of nitems share matrices [n][nchunks], item i at element i * item_stride of shares_d
        (default n * nchunks: back to back), with one scan and one decoder launch for all of them.  Returns ONE RobustUnpack
        with an item axis: status and errpos are [nitems][nchunks] (`nchunks` of the report counts all of them), `summaries`
        holds one summary per item, `nitems` is set and `out` is shares_d.
        With `parties` (ascending ids, one list for all items) every item is a compact matrix [len(parties)][nchunks] as
        repair(parties=...) takes it (default stride len(parties) * nchunks) and the call is zk_pss_repair_batch_parties."""
        k = 2 * self.l if dimension is None else int(dimension)
        rows = self.n if parties is None else len(parties)
        stride = rows * nchunks if item_stride is None else int(item_stride)
        r = self._report(max(0, nitems) * nchunks, k, parties, words=max(1, nitems))
        r.out, r.nitems = shares_d, nitems
        if parties is None:
            self._check(self.lib.zk_pss_repair_batch(self.h, _ptr(shares_d), stride, nitems, nchunks, k, _ptr(r.status),
                                                     _ptr(r.errpos), _ptr(r.summary_d), stream))
        else:
            arr = (C.c_uint32 * len(r.parties))(*r.parties)
            self._check(self.lib.zk_pss_repair_batch_parties(self.h, _ptr(shares_d), arr, len(r.parties), stride, nitems,
                                                             nchunks, k, _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d),
                                                             stream))
        return r

    def unpack_points_robust(self, group, shares_d, nchunks, dimension=None, want_out=True, stream=None, parties=None):
        """zk_pss_unpack_points_robust: the robust unpack of all n parties' packed POINT shares [n][nchunks] affine (pss.rs:125-166
        over group elements).  One wrong share per chunk is located and corrected when n - dimension >= 2; at dimension
        4l - 1 the call only detects.  dimension: 2l (the default) up to 4l - 1.  Returns a RobustUnpack with status, errpos
        and summary; `out` is [nchunks][l] affine (None with want_out=False): the unpack of the clean or corrected word,
        identities for a failed chunk.
        With `parties` (ascending ids) shares_d is the compact [len(parties)][nchunks], the other parties are absent and the call
        is zk_pss_unpack_points_robust_parties: one wrong share is corrected when len(parties) - dimension >= 2, errpos and the
        summary go by party id."""
        k = 2 * self.l if dimension is None else int(dimension)
        r = self._report(nchunks, k, parties)
        width = self.fq.nl * (4 if group == ZK_G2 else 2) * 8
        r.out = DeviceBuffer(self, max(1, nchunks * self.l) * width) if want_out else None
        if parties is None:
            self._check(self.lib.zk_pss_unpack_points_robust(self.h, group, _ptr(shares_d), nchunks, k, _ptr(r.out),
                                                             _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        else:
            arr = (C.c_uint32 * len(r.parties))(*r.parties)
            self._check(self.lib.zk_pss_unpack_points_robust_parties(self.h, group, _ptr(shares_d), arr, len(r.parties), nchunks,
                                                                     k, _ptr(r.out), _ptr(r.status), _ptr(r.errpos),
                                                                     _ptr(r.summary_d), stream))
        return r

    def repair_points(self, group, shares_d, nchunks, dimension=None, stream=None, parties=None):
        """zk_pss_repair_points: unpack_points_robust's verdicts written back into shares_d [n][nchunks] affine, in place: in a
        corrected chunk the one share errpos names becomes the honest one, every other element keeps its bytes.  Returns a
        RobustUnpack with status, errpos and summary; `out` is shares_d.
        With `parties` (ascending ids) shares_d is the compact [len(parties)][nchunks] and the call is
        zk_pss_repair_points_parties: a named party's share is written at its row, an absent party's is not recovered."""
        k = 2 * self.l if dimension is None else int(dimension)
        r = self._report(nchunks, k, parties)
        r.out = shares_d
        if parties is None:
            self._check(self.lib.zk_pss_repair_points(self.h, group, _ptr(shares_d), nchunks, k, _ptr(r.status), _ptr(r.errpos),
                                                      _ptr(r.summary_d), stream))
        else:
            arr = (C.c_uint32 * len(r.parties))(*r.parties)
            self._check(self.lib.zk_pss_repair_points_parties(self.h, group, _ptr(shares_d), arr, len(r.parties), nchunks, k,
                                                              _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r

    def d_msm_checked(self, group, bases_d, scalars_d, length, msm_mask=None, stream=None):
        """zk_d_msm_checked: d_msm with the king's word msm_p + in_mask_p checked at dimension 4l - 1 (detection only).
        Returns (out, status): out as d_msm's, [n][3 * coord limbs] Jacobian; status 0 (the word is a codeword) or 2."""
        msm_mask = msm_mask or MsmMask.zero()
        nl = self.fq.nl * (2 if group == ZK_G2 else 1)
        out = np.zeros((self.n, 3 * nl), dtype=np.uint64)
        status = C.c_uint8(255)
        im = None if msm_mask.in_mask is None else np.ascontiguousarray(msm_mask.in_mask, dtype=np.uint64)
        om = None if msm_mask.out_mask is None else np.ascontiguousarray(msm_mask.out_mask, dtype=np.uint64)
        self._check(self.lib.zk_d_msm_checked(self.h, group, _ptr(bases_d), _ptr(scalars_d), length,
                                              None if im is None else im.ctypes.data, None if om is None else om.ctypes.data,
                                              out.ctypes.data, C.addressof(status), stream))
        return out, status.value

    def lagrange_unpack(self, shares_d, nchunks, parties, out=None, stream=None):
        return self.unpack2(shares_d, nchunks, parties, out, stream)

    unpack_missing_shares = unpack2


class RobustUnpack:
    """Result of PackedSharingParams.unpack_robust, and the report of PackedSharingParams.repair and of the checked king rounds
    (d_fft / d_ifft / deg_red / fft2_king with check=True), which leave secrets and message None and set `out` to the buffer
    that holds the call's result.  Device buffers: secrets [nchunks * l] (order 0), status [nchunks] bytes
    (0 clean, 1 corrected, 2 failed), errpos [nchunks] u32 (bit p: party p's share was corrected), summary_d [3 + n] u64,
    message [dimension][nchunks] or None.  `summary` downloads summary_d: [clean, corrected, failed] + per party the number
    of chunks in which its share was corrected.  `parties`: the party list the call was given, None for all n.
    d_pp with check=True checks two words, num then den: status and errpos are [2 * length] in that order, summary_d is
    [2][3 + n], `summary` is num's and `summaries` holds both."""
    CLEAN, CORRECTED, FAILED = 0, 1, 2

    def __init__(self, ctx, nchunks, dimension, parties=None):
        self.ctx, self.nchunks, self.dimension, self.parties = ctx, nchunks, dimension, parties
        self.secrets = self.status = self.errpos = self.summary_d = self.message = self.out = None

    @property
    def summary(self):
        if not self.nchunks:            # the call writes nothing for an empty vector
            return [0] * (3 + self.ctx.n)
        return [int(v) for v in self.summary_d.to_numpy(np.uint64)[:3 + self.ctx.n]]

    @property
    def summaries(self):
        """one summary per word the call checked"""
        w = 3 + self.ctx.n
        if not self.nchunks:
            return [[0] * w for _ in range(self.summary_d.nbytes // (8 * w))]
        flat = [int(v) for v in self.summary_d.to_numpy(np.uint64)]
        return [flat[i:i + w] for i in range(0, len(flat) - w + 1, w)]

    def status_host(self):
        return self.status.to_numpy(np.uint8) if self.nchunks else np.zeros(0, np.uint8)

    def errpos_host(self):
        return self.errpos.to_numpy(np.uint32) if self.nchunks else np.zeros(0, np.uint32)


class FftMask:
    """dist-primitives/src/dfft/mod.rs:16-95; buffers are [n][m/l] for all parties."""

    def __init__(self, in_mask, out_mask):
        self.in_mask, self.out_mask = in_mask, out_mask

    @staticmethod
    def sample(pp, rearrange, g, inverse, log2_m, seed, stream=None):
        cnt = pp.n * ((1 << log2_m) // pp.l)
        im, om = pp.alloc_fr(cnt), pp.alloc_fr(cnt)
        gp = None if g is None else pp.fr.encode_one(g).ctypes.data
        garr = None if g is None else pp.fr.encode_one(g)
        pp._check(pp.lib.zk_fft_mask_sample(pp.h, int(rearrange), None if garr is None else garr.ctypes.data,
                                            int(inverse), log2_m, seed, im.ptr, om.ptr, stream))
        del gp
        return FftMask(im, om)

    @staticmethod
    def zero():
        return FftMask(None, None)


class DegRedMask:
    """dist-primitives/src/utils/deg_red.rs:14-77 over Fr."""

    def __init__(self, in_mask, out_mask):
        self.in_mask, self.out_mask = in_mask, out_mask

    @staticmethod
    def sample(pp, num, seed, stream=None):
        im, om = pp.alloc_fr(pp.n * num), pp.alloc_fr(pp.n * num)
        pp._check(pp.lib.zk_degred_mask_sample(pp.h, num, seed, im.ptr, om.ptr, stream))
        return DegRedMask(im, om)

    @staticmethod
    def zero():
        return DegRedMask(None, None)


class MsmMask:
    """dist-primitives/src/dmsm/mod.rs:10-57: n Jacobian points each (host numpy arrays) or None."""

    def __init__(self, in_mask=None, out_mask=None):
        self.in_mask, self.out_mask = in_mask, out_mask

    @staticmethod
    def zero():
        return MsmMask(None, None)

    @staticmethod
    def sample(pp, group, gen_affine, seed):
        """MsmMask::sample (dmsm/mod.rs:21-47); gen_affine: the group generator as Montgomery limbs (uint64 array)."""
        nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
        gen = np.ascontiguousarray(gen_affine, dtype=np.uint64).reshape(-1)
        if gen.size != 2 * nl:
            raise ValueError("generator must be an affine point (%d limbs)" % (2 * nl))
        im = np.zeros((pp.n, 3 * nl), dtype=np.uint64)
        om = np.zeros((pp.n, 3 * nl), dtype=np.uint64)
        pp._check(pp.lib.zk_msm_mask_sample(pp.h, group, gen.ctypes.data, seed, im.ctypes.data, om.ctypes.data))
        return MsmMask(im, om)


BASE_MUL_FEW_MAX = 4096       # zk_base_mul_few's bound on the number of scalars (zk_base_mul above it)


def base_mul_few(pp, group, base_affine, scalars_d, length, out=None, stream=None):
    """zk_base_mul_few: scalars_d[i] * base for a FEW scalars (at most BASE_MUL_FEW_MAX), a group of lanes per scalar;
    base_affine: Montgomery limbs of an affine point (host).  Returns a DeviceBuffer of `length` Jacobian points."""
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    base = np.ascontiguousarray(base_affine, dtype=np.uint64).reshape(-1)
    if base.size != 2 * nl:
        raise ValueError("base must be an affine point (%d limbs)" % (2 * nl))
    out = out or DeviceBuffer(pp, max(1, length) * 3 * nl * 8)
    pp._check(pp.lib.zk_base_mul_few(pp.h, group, base.ctypes.data, _ptr(scalars_d), length, _ptr(out), stream))
    return out


H_ITEMS = 7                   # the king words of circom_h: three of d_ifft, three of d_fft, one of deg_red


def h_report(pp, log2_m):
    """the report buffers of zk_circom_h_checked / zk_groth16_prove_checked: a RobustUnpack with an item axis, status and
    errpos [7][m/l], one summary per item in `summaries` (items 0..5 at dimension 2l, item 6 at 4l - 1: detection only)"""
    lc = (1 << log2_m) // pp.l
    r = pp._report(H_ITEMS * lc, 2 * pp.l, words=H_ITEMS)
    r.nitems = H_ITEMS
    return r


def circom_h(pp, wit_or_bufs, masks=None, seed=0, check=False, log2_m=None, stream=None, parties=None):
    """zk_circom_h (ext_wit.rs:104-181) on the QAP share vectors of a Witness (`.qap`, `.log_m`) or on three device buffers
    [n][m/l] with log2_m given.  masks: a zk_groth16_masks structure, an object that holds one as `.ct`, or None.
    Returns h [n][m/l]; with check=True zk_circom_h_checked and (h, report), the report as h_report's.
    parties (with check=True only; ascending ids, all n or n - 1 of them): zk_circom_h_checked_parties -- only the listed
    parties' words reach the kings, the rows of the absent party in every input and in-mask are not read; with n - 1
    parties item 6 is not checked and its summary is all zeros."""
    if parties is not None and not check:
        raise ValueError("a party list needs check=True (the unchecked chain takes all n parties)")
    if hasattr(wit_or_bufs, "qap"):
        qap, log2_m = wit_or_bufs.qap, wit_or_bufs.log_m
    else:
        qap = list(wit_or_bufs)
    if log2_m is None or len(qap) != 3:
        raise ValueError("three QAP share vectors and log2_m")
    masks = getattr(masks, "ct", masks)
    mk = None if masks is None else C.byref(masks)
    h = pp.alloc_fr(pp.n * ((1 << log2_m) // pp.l))
    if not check:
        pp._check(pp.lib.zk_circom_h(pp.h, _ptr(qap[0]), _ptr(qap[1]), _ptr(qap[2]), log2_m, mk, seed, h.ptr, stream))
        return h
    rep = h_report(pp, log2_m)
    rep.out = h
    if parties is None:
        pp._check(pp.lib.zk_circom_h_checked(pp.h, _ptr(qap[0]), _ptr(qap[1]), _ptr(qap[2]), log2_m, mk, seed, h.ptr,
                                             _ptr(rep.status), _ptr(rep.errpos), _ptr(rep.summary_d), stream))
    else:
        rep.parties = list(parties)
        arr = (C.c_uint32 * len(rep.parties))(*rep.parties)
        pp._check(pp.lib.zk_circom_h_checked_parties(pp.h, arr, len(rep.parties), _ptr(qap[0]), _ptr(qap[1]), _ptr(qap[2]),
                                                     log2_m, mk, seed, h.ptr, _ptr(rep.status), _ptr(rep.errpos),
                                                     _ptr(rep.summary_d), stream))
    return h, rep


def h_batch_reports(pp, nproofs, log2_m):
    """the report buffers of zk_circom_h_batch_checked / zk_groth16_prove_checked_batch: status and errpos [nproofs][7][m/l],
    summary [nproofs][7][3 + n], proof-major.  Returns (whole, reports): `whole` owns the buffers the call is given,
    reports[b] is proof b's slice as windows into them, shaped exactly like h_report's."""
    lc = (1 << log2_m) // pp.l
    rows = H_ITEMS * lc
    whole = pp._report(nproofs * rows, 2 * pp.l, words=nproofs * H_ITEMS)
    whole.nitems = nproofs * H_ITEMS
    reports = []
    for b in range(nproofs):
        r = RobustUnpack(pp, rows, 2 * pp.l)
        r.status = whole.status.view(b * rows, rows)
        r.errpos = whole.errpos.view(4 * b * rows, 4 * rows)
        sw = 8 * (3 + pp.n) * H_ITEMS
        r.summary_d = whole.summary_d.view(b * sw, sw)
        r.nitems = H_ITEMS
        reports.append(r)
    return whole, reports


def circom_h_batch_checked(pp, wits_or_bufs, masks=None, seed=0, log2_m=None, stream=None, errpos=True, summary=True):
    """zk_circom_h_batch_checked: the checked h chain of len(wits_or_bufs) proofs (1..16) as one launch chain.  Each entry is a
    Witness (`.qap`, `.log_m`) or three device buffers [n][m/l] with log2_m given; masks: one zk_groth16_masks (or an object
    holding one as `.ct`) per proof, or None.  Proof b is circom_h(check=True) with seed + 16 b.  Returns (hs, reports):
    hs[b] a window [n][m/l] into one buffer, reports[b] as h_report's (errpos=False / summary=False pass NULL for that
    buffer: the slices are then not written)."""
    nb = len(wits_or_bufs)
    qaps = []
    for w in wits_or_bufs:
        if hasattr(w, "qap"):
            qaps.append(w.qap)
            log2_m = w.log_m
        else:
            qaps.append(list(w))
    if log2_m is None or any(len(q) != 3 for q in qaps):
        raise ValueError("three QAP share vectors per proof and log2_m")
    if masks is not None and len(masks) != nb:
        raise ValueError("one mask set per proof")
    mk = None
    if masks is not None:
        ct = [getattr(m, "ct", m) for m in masks]
        mk = (type(ct[0]) * nb)()
        for b, m in enumerate(ct):
            C.memmove(C.byref(mk, b * C.sizeof(m)), C.byref(m), C.sizeof(m))
    per = pp.n * ((1 << log2_m) // pp.l)
    h = pp.alloc_fr(max(1, nb) * per)
    whole, reports = h_batch_reports(pp, max(1, nb), log2_m)
    arr = lambda k: (C.c_void_p * max(1, nb))(*[_ptr(q[k]) for q in qaps])
    pp._check(pp.lib.zk_circom_h_batch_checked(pp.h, nb, arr(0), arr(1), arr(2), log2_m,
                                               None if mk is None else C.cast(mk, C.c_void_p), seed, h.ptr, _ptr(whole.status),
                                               _ptr(whole.errpos) if errpos else None,
                                               _ptr(whole.summary_d) if summary else None, stream))
    esz = h.nbytes // (max(1, nb) * per)
    return [h.view(b * per * esz, per * esz) for b in range(nb)], reports


def deal_masks(pp, nproofs, log2_m, g1_gen_affine, g2_gen_affine, seed, masks_ct, stream=None):
    """zk_groth16_deal_masks: fills the destination buffers named by `masks_ct` (a ctypes array of nproofs
    zk_groth16_masks, or one struct when nproofs == 1) with the twelve masks of every proof; proof b is dealt what the
    single samplers deal with seed + 16 b (replay mode).  A slot with two NULL pointers is skipped.  Returns with the
    host points written and the device masks ordered on `stream`."""
    g1 = None if g1_gen_affine is None else np.ascontiguousarray(g1_gen_affine, dtype=np.uint64).reshape(-1)
    g2 = None if g2_gen_affine is None else np.ascontiguousarray(g2_gen_affine, dtype=np.uint64).reshape(-1)
    pp._check(pp.lib.zk_groth16_deal_masks(pp.h, nproofs, log2_m, None if g1 is None else g1.ctypes.data,
                                           None if g2 is None else g2.ctypes.data, seed, C.byref(masks_ct), stream))


def fft2_king(pp, in_d, log2_m, inverse=False, g=None, scale_size_inv=False, rearrange=False, seed=0, out=None, out_mask=None,
              parties=None, check=False, stream=None):
    """zk_fft2_king, the king of d_fft / d_ifft (dfft/mod.rs:264-304) on in_d [nparties][m/l]; never in place.  Returns `out`.
    check=True (all n parties): zk_fft2_king_checked -- in_d is repaired in place first (dimension 2l); returns the report, a
    RobustUnpack whose `out` is the output buffer."""
    out = out or pp.alloc_fr(pp.n * ((1 << log2_m) // pp.l))
    garr = None if g is None else pp.fr.encode_one(g)
    gp = None if garr is None else garr.ctypes.data
    arr, np_ = (None, pp.n) if parties is None else ((C.c_uint32 * len(parties))(*parties), len(parties))
    if not check:
        pp._check(pp.lib.zk_fft2_king(pp.h, _ptr(in_d), arr, np_, log2_m, int(inverse), gp, int(scale_size_inv), int(rearrange),
                                      seed, _ptr(out), _ptr(out_mask), stream))
        return out
    r = pp._report((1 << log2_m) // pp.l, 2 * pp.l)
    r.out = out
    pp._check(pp.lib.zk_fft2_king_checked(pp.h, _ptr(in_d), arr, np_, log2_m, int(inverse), gp, int(scale_size_inv),
                                          int(rearrange), seed, _ptr(out), _ptr(out_mask), _ptr(r.status), _ptr(r.errpos),
                                          _ptr(r.summary_d), stream))
    return r


def fft2_king_checked_parties(pp, in_d, parties, log2_m, inverse=False, g=None, scale_size_inv=False, rearrange=False, seed=0,
                              out=None, out_mask=None, stream=None):
    """zk_fft2_king_checked_parties: in_d [len(parties)][m/l], the words of the listed parties (ascending ids; None: all n),
    is repaired in place with the list (dimension 2l, up to (len(parties) - 2l) // 2 wrong shares per chunk), then the king
    runs with the same list; never in place.  Returns the report, a RobustUnpack whose `out` is the output buffer [n][m/l]."""
    out = out or pp.alloc_fr(pp.n * ((1 << log2_m) // pp.l))
    garr = None if g is None else pp.fr.encode_one(g)
    gp = None if garr is None else garr.ctypes.data
    arr, np_ = (None, pp.n) if parties is None else ((C.c_uint32 * len(parties))(*parties), len(parties))
    r = pp._report((1 << log2_m) // pp.l, 2 * pp.l, parties)
    r.out = out
    pp._check(pp.lib.zk_fft2_king_checked_parties(pp.h, _ptr(in_d), arr, np_, log2_m, int(inverse), gp, int(scale_size_inv),
                                                  int(rearrange), seed, _ptr(out), _ptr(out_mask), _ptr(r.status),
                                                  _ptr(r.errpos), _ptr(r.summary_d), stream))
    return r


def d_fft(pp, shares_d, fft_mask, rearrange, log2_m, seed=0, out=None, stream=None, check=False, parties=None):
    """dfft/mod.rs:99-134 for all parties; shares_d [n][m/l].  Result in `out` (or back in shares_d if None).
    check=True: zk_d_fft_checked -- the word the king receives is repaired first (up to l wrong parties per chunk); returns
    the report, a RobustUnpack whose `out` is the buffer with the result.  With `parties` (ascending ids; check=True only)
    the call is zk_d_fft_checked_parties: only the listed rows of shares_d and of the in-mask reach the king."""
    if parties is not None and not check:
        raise ValueError("a party list is the checked call's: pass check=True")
    if check and parties is not None:
        r = pp._report((1 << log2_m) // pp.l, 2 * pp.l, parties)
        r.out = shares_d if out is None else out
        arr = (C.c_uint32 * len(r.parties))(*r.parties)
        pp._check(pp.lib.zk_d_fft_checked_parties(pp.h, _ptr(shares_d), arr, len(r.parties), _ptr(fft_mask.in_mask),
                                                  _ptr(fft_mask.out_mask), int(rearrange), log2_m, seed, _ptr(out),
                                                  _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    if check:
        r = pp._report((1 << log2_m) // pp.l, 2 * pp.l)
        r.out = shares_d if out is None else out
        pp._check(pp.lib.zk_d_fft_checked(pp.h, _ptr(shares_d), _ptr(fft_mask.in_mask), _ptr(fft_mask.out_mask), int(rearrange),
                                          log2_m, seed, _ptr(out), _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    pp._check(pp.lib.zk_d_fft(pp.h, _ptr(shares_d), _ptr(fft_mask.in_mask), _ptr(fft_mask.out_mask), int(rearrange),
                              log2_m, seed, _ptr(out), stream))
    return shares_d if out is None else out


def d_ifft(pp, shares_d, fft_mask, rearrange, log2_m, g=None, seed=0, out=None, stream=None, check=False, parties=None):
    """dfft/mod.rs:137-175; g is an int (coset shift, 1 if None).  check=True: zk_d_ifft_checked, as d_fft's; with `parties`
    zk_d_ifft_checked_parties."""
    garr = None if g is None else pp.fr.encode_one(g)
    if parties is not None and not check:
        raise ValueError("a party list is the checked call's: pass check=True")
    if check and parties is not None:
        r = pp._report((1 << log2_m) // pp.l, 2 * pp.l, parties)
        r.out = shares_d if out is None else out
        arr = (C.c_uint32 * len(r.parties))(*r.parties)
        pp._check(pp.lib.zk_d_ifft_checked_parties(pp.h, _ptr(shares_d), arr, len(r.parties), _ptr(fft_mask.in_mask),
                                                   _ptr(fft_mask.out_mask), int(rearrange), log2_m,
                                                   None if garr is None else garr.ctypes.data, seed, _ptr(out),
                                                   _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    if check:
        r = pp._report((1 << log2_m) // pp.l, 2 * pp.l)
        r.out = shares_d if out is None else out
        pp._check(pp.lib.zk_d_ifft_checked(pp.h, _ptr(shares_d), _ptr(fft_mask.in_mask), _ptr(fft_mask.out_mask),
                                           int(rearrange), log2_m, None if garr is None else garr.ctypes.data, seed, _ptr(out),
                                           _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    pp._check(pp.lib.zk_d_ifft(pp.h, _ptr(shares_d), _ptr(fft_mask.in_mask), _ptr(fft_mask.out_mask), int(rearrange),
                               log2_m, None if garr is None else garr.ctypes.data, seed, _ptr(out), stream))
    return shares_d if out is None else out


def deg_red(pp, x_d, mask, length, seed=0, stream=None, check=False):
    """utils/deg_red.rs:80-126 over Fr; x_d [n][length] in place.  check=True: zk_deg_red_checked -- detection only (the
    word x + in_mask has dimension 4l - 1: a status is 0 or 2 and nothing is rewritten); returns the report, `out` is x_d."""
    if check:
        r = pp._report(length, 4 * pp.l - 1)
        r.out = x_d
        pp._check(pp.lib.zk_deg_red_checked(pp.h, _ptr(x_d), _ptr(mask.in_mask), _ptr(mask.out_mask), length, seed,
                                            _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    pp._check(pp.lib.zk_deg_red(pp.h, _ptr(x_d), _ptr(mask.in_mask), _ptr(mask.out_mask), length, seed, stream))
    return x_d


def d_pp(pp, num_d, den_d, mask, length, seed=0, out=None, stream=None, check=False, parties=None):
    """dpp/mod.rs:15-87; num_d, den_d [n][length].  check=True: zk_d_pp_checked -- the king's word num ++ den is repaired
    first, num_d and den_d IN PLACE (dimension 2l); with `parties` (ascending ids) they are [len(parties)][length], the
    words of the listed parties.  Returns the report, a RobustUnpack over 2 * length chunks (num's, then den's) whose
    `summaries` are num's and den's and whose `out` is the result [n][length]."""
    out = out or pp.alloc_fr(pp.n * length)
    if parties is not None and not check:
        raise ValueError("a party list is the checked call's: pass check=True")
    if check:
        r = pp._report(2 * length, 2 * pp.l, parties, words=2)
        r.out = out
        arr, np_ = (None, pp.n) if parties is None else ((C.c_uint32 * len(r.parties))(*r.parties), len(r.parties))
        pp._check(pp.lib.zk_d_pp_checked(pp.h, _ptr(num_d), _ptr(den_d), arr, np_, _ptr(mask.in_mask), _ptr(mask.out_mask),
                                         length, seed, _ptr(out), _ptr(r.status), _ptr(r.errpos), _ptr(r.summary_d), stream))
        return r
    pp._check(pp.lib.zk_d_pp(pp.h, _ptr(num_d), _ptr(den_d), _ptr(mask.in_mask), _ptr(mask.out_mask), length, seed,
                             _ptr(out), stream))
    return out


def msm(pp, group, bases_d, scalars_d, length, len_scalars=None, stream=None):
    """G::msm (dmsm/mod.rs:73): returns one Jacobian point as a uint64 array [3 * coord limbs]."""
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    out = np.zeros(3 * nl, dtype=np.uint64)
    ls = length if len_scalars is None else len_scalars
    pp._check(pp.lib.zk_msm(pp.h, group, _ptr(bases_d), length, _ptr(scalars_d), ls, out.ctypes.data, stream))
    return out


def msm_batch(pp, group, bases_d, scalar_vectors, length, stream=None):
    """zk_msm_batch: ONE base vector against several scalar vectors (G::msm once per witness, one Pippenger pass):
    returns [nvec][3 * coord limbs] Jacobian points."""
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    nv = len(scalar_vectors)
    out = np.zeros((nv, 3 * nl), dtype=np.uint64)
    arr = (C.c_void_p * nv)(*[_ptr(v) for v in scalar_vectors])
    pp._check(pp.lib.zk_msm_batch(pp.h, group, _ptr(bases_d), length, arr, nv, out.ctypes.data, stream))
    return out


def msm_stats(pp):
    """zk_msm_stats: the context's running counts [G1 mixed additions, G2 mixed additions, G1 (point, window) pairs offered
    to the sorts, G2 pairs offered]."""
    st = (C.c_uint64 * 4)()
    pp._check(pp.lib.zk_msm_stats(pp.h, st))
    return list(st)


def msm_sum(pp, group, triples, stream=None, with_shared=False):
    """zk_msm_sum: the sum of up to three MSMs [(bases_d, scalars_d, length), ...] over one group as ONE Jacobian point,
    through one shared bucket set where the launches' geometries match.  with_shared: also how many of the first k - 1
    launches shared the last one's bucket set."""
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    k = len(triples)
    out = np.zeros(3 * nl, dtype=np.uint64)
    ba = (C.c_void_p * k)(*[_ptr(t[0]) for t in triples])
    sa = (C.c_void_p * k)(*[_ptr(t[1]) for t in triples])
    la = (C.c_size_t * k)(*[int(t[2]) for t in triples])
    shared = C.c_int32(0)
    pp._check(pp.lib.zk_msm_sum(pp.h, group, k, ba, sa, la, out.ctypes.data, C.byref(shared), stream))
    return (out, shared.value) if with_shared else out


def unpack_points(pp, group, shares_d, nchunks, parties=None, two=True, out=None, stream=None):
    """pss.rs:125-166 over group elements: shares_d [nparties][nchunks] affine -> [nchunks][l] affine (device).
    two=False: unpack (all n parties); parties: ascending ids of the shares present (lagrange_unpack)."""
    width = pp.fq.nl * (4 if group == ZK_G2 else 2) * 8
    out = out or DeviceBuffer(pp, nchunks * pp.l * width)
    if not two:
        pp._check(pp.lib.zk_pss_unpack_points(pp.h, group, _ptr(shares_d), nchunks, _ptr(out), stream))
        return out
    if parties is None:
        pp._check(pp.lib.zk_pss_unpack2_points(pp.h, group, _ptr(shares_d), None, pp.n, nchunks, _ptr(out), stream))
    else:
        ids = (C.c_uint32 * len(parties))(*parties)
        pp._check(pp.lib.zk_pss_unpack2_points(pp.h, group, _ptr(shares_d), ids, len(parties), nchunks, _ptr(out), stream))
    return out


def fr_to_bytes(pp, x_d, count, stream=None):
    """ark-serialize CanonicalSerialize of `count` Fr elements of a device vector: bytes (32 or 48 per element,
    little-endian canonical integers) -- the payload of an mpc-net frame (ser_net.rs:24-25)."""
    out = pp.alloc_fr(count)
    pp._check(pp.lib.zk_fr_to_bytes(pp.h, _ptr(x_d), count, out.ptr, stream))
    pp.sync(stream)
    return out.to_numpy(dtype=np.uint8)[: count * pp.fr.nbytes].tobytes()


def fr_from_bytes(pp, data, stream=None):
    """CanonicalDeserialize of a byte string of Fr elements into a device vector (Montgomery form); raises if an
    element is not below the modulus, as arkworks does."""
    nb = pp.fr.nbytes
    host = (np.ascontiguousarray(data).view(np.uint8).reshape(-1) if isinstance(data, np.ndarray)
            else np.frombuffer(data, dtype=np.uint8))
    if host.size % nb:
        raise ValueError("byte length is not a multiple of the element size")
    count = host.size // nb
    raw = DeviceBuffer.from_numpy(pp, host)
    out = pp.alloc_fr(max(count, 1))
    pp._check(pp.lib.zk_fr_from_bytes(pp.h, raw.ptr, count, out.ptr, stream))
    return out


def msm_precompute(pp, group, bases_d, length, stream=None):
    """zk_msm_precompute: fixed-base table for the affine vector bases_d [length]; later MSMs over it use the table."""
    pp._check(pp.lib.zk_msm_precompute(pp.h, group, _ptr(bases_d), length, stream))


def msm_forget(pp, bases_d):
    pp._check(pp.lib.zk_msm_forget(pp.h, _ptr(bases_d)))


def msm_table_info(pp, group, bases_d):
    import ctypes as C
    info = (C.c_int * 2)()
    pp._check(pp.lib.zk_msm_table_info(pp.h, group, _ptr(bases_d), info))
    return {"window_bits": info[0], "windows": info[1]}


# Base-field Montgomery products (one product = 2 N^2 + N multiply instructions: 136 v_mad_u64_u32 for 8 limbs) that ONE mixed
# XYZZ addition of the accumulate kernels costs, counted in multiply instructions (csrc/field.hpp):
#   G1: 8 products + Y3 = R (Q - X3) - Y1 PPP as one pass with one reduction (3 N^2 + N)      -> 1288 / 136 = 9.47
#   G2: 8 Fq2 products with lazy reduction (3 N^2 + 2 (N^2 + N) = 336) + 2 Fq2 squarings (272)   -> 3232 / 136 = 23.76
# (the textbook counts are 10 and 28; the accounting of bench.py uses what the kernels execute)
MULS_PER_ADD = {ZK_G1: 1288 / 136, ZK_G2: 3232 / 136}


def msm_plan(pp, group, length):
    """The Pippenger plan zk_msm uses for `length` points: dict(window_bits, windows, lane_points, muls_per_add,
    muls_per_add_textbook); muls_per_add = base-field products per mixed addition as executed (MULS_PER_ADD)."""
    import ctypes as C
    plan = (C.c_int * 4)()
    pp._check(pp.lib.zk_msm_plan(pp.h, group, length, plan))
    return {"window_bits": plan[0], "windows": plan[1], "lane_points": plan[2],
            "muls_per_add": round(MULS_PER_ADD[group], 2), "muls_per_add_textbook": plan[3]}


def d_msm(pp, group, bases_d, scalars_d, length, msm_mask=None, stream=None):
    """dmsm/mod.rs:59-102 for all parties: bases_d [n][length] affine, scalars_d [n][length].
    Returns the n parties' output shares as a uint64 array [n][3 * coord limbs] (Jacobian)."""
    msm_mask = msm_mask or MsmMask.zero()
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    out = np.zeros((pp.n, 3 * nl), dtype=np.uint64)
    im = None if msm_mask.in_mask is None else np.ascontiguousarray(msm_mask.in_mask, dtype=np.uint64)
    om = None if msm_mask.out_mask is None else np.ascontiguousarray(msm_mask.out_mask, dtype=np.uint64)
    pp._check(pp.lib.zk_d_msm(pp.h, group, _ptr(bases_d), _ptr(scalars_d), length,
                              None if im is None else im.ctypes.data, None if om is None else om.ctypes.data,
                              out.ctypes.data, stream))
    return out


def deg_red_parties(pp, x_d, parties, mask, length, seed=0, out=None, stream=None):
    """deg_red when only `parties` reached the king (ser_net.rs:57-94 -> pss.rs:170-221); x_d [len(parties)][length]."""
    out = out or pp.alloc_fr(pp.n * length)
    arr = (C.c_uint32 * len(parties))(*parties)
    pp._check(pp.lib.zk_deg_red_parties(pp.h, _ptr(x_d), arr, len(parties), _ptr(mask.in_mask), _ptr(mask.out_mask),
                                        length, seed, _ptr(out), stream))
    return out


def d_msm_parties(pp, group, bases_d, scalars_d, length, parties, msm_mask=None, stream=None):
    """d_msm when only `parties` reached the king; bases_d / scalars_d [len(parties)][length]."""
    msm_mask = msm_mask or MsmMask.zero()
    nl = pp.fq.nl * (2 if group == ZK_G2 else 1)
    out = np.zeros((pp.n, 3 * nl), dtype=np.uint64)
    arr = (C.c_uint32 * len(parties))(*parties)
    im = None if msm_mask.in_mask is None else np.ascontiguousarray(msm_mask.in_mask, dtype=np.uint64)
    om = None if msm_mask.out_mask is None else np.ascontiguousarray(msm_mask.out_mask, dtype=np.uint64)
    pp._check(pp.lib.zk_d_msm_parties(pp.h, group, _ptr(bases_d), _ptr(scalars_d), length, arr, len(parties),
                                      None if im is None else im.ctypes.data, None if om is None else om.ctypes.data,
                                      out.ctypes.data, stream))
    return out


def vec_scale(pp, x_d, k, length, stream=None):
    karr = pp.fr.encode_one(k)
    pp._check(pp.lib.zk_vec_scale(pp.h, _ptr(x_d), karr.ctypes.data, length, stream))
    return x_d


def vec_mul_sub(pp, out_d, a_d, b_d, c_d, length, stream=None):
    pp._check(pp.lib.zk_vec_mul_sub(pp.h, _ptr(out_d), _ptr(a_d), _ptr(b_d), _ptr(c_d), length, stream))
    return out_d


FQ12_OPS = {"mul": 0, "sqr": 1, "inverse": 2, "conj": 3, "frobenius1": 4, "frobenius2": 5, "frobenius3": 6,
            "cyclotomic_sqr": 7, "line_mul": 8}


def multi_pairing(pp, p_affine_d, q_affine_d, k, count, out=None, stream=None):
    """zk_multi_pairing (ark-ec Pairing::multi_pairing): out[i] = final_exp(prod_j miller(P[i][j], Q[i][j])) for
    [count][k] affine G1 / G2 points on the device.  Returns a DeviceBuffer of [count][12] Fq (Montgomery) in the
    coefficient order of arkworks' Fp12."""
    out = out or DeviceBuffer(pp, max(1, count) * 12 * pp.fq.nbytes)
    pp._check(pp.lib.zk_multi_pairing(pp.h, _ptr(p_affine_d), _ptr(q_affine_d), k, count, out.ptr, stream))
    return out


def fq12_selftest(pp, op, a_d, b_d, length, out=None, stream=None):
    """zk_fq12_selftest: one operation of the lane-split Fq12 tower on [length][12] Fq; op is a key of FQ12_OPS."""
    out = out or DeviceBuffer(pp, max(1, length) * 12 * pp.fq.nbytes)
    pp._check(pp.lib.zk_fq12_selftest(pp.h, FQ12_OPS[op] if isinstance(op, str) else int(op), _ptr(a_d), _ptr(b_d), length,
                                      out.ptr, stream))
    return out


def points_subgroup_check(pp, group, affine_d, length, out=None, stream=None):
    """zk_points_subgroup_check (ark-ec is_in_correct_subgroup_assuming_on_curve after the curve test): one byte per affine
    Montgomery point of the device vector [length] -- 1 when both coordinates are below q and the point is the identity
    (0, 0) or lies in the order-r subgroup, 0 otherwise (also for a point off its curve).  Returns a uint8 array."""
    out = out or DeviceBuffer(pp, max(1, length))
    pp._check(pp.lib.zk_points_subgroup_check(pp.h, group, _ptr(affine_d), length, out.ptr, stream))
    return out.to_numpy(dtype=np.uint8)[:length].copy()


def points_decompress_checked(pp, group, bytes_d, length, out=None, stream=None):
    """zk_points_decompress_checked (CanonicalDeserialize::deserialize_compressed with validation, per element): decodes as
    zk_points_decompress does and tests the subgroup.  Returns (points, ok): the device vector of affine Montgomery points
    and a uint8 array -- ok[i] = 0 with (0, 0) written for an invalid encoding, ok[i] = 0 with the decoded point kept for a
    point outside the subgroup.  A bad element never fails the call."""
    size = pp.fq.nbytes * (4 if group == ZK_G2 else 2)
    out = out or DeviceBuffer(pp, max(1, length) * size)
    ok = DeviceBuffer(pp, max(1, length))
    pp._check(pp.lib.zk_points_decompress_checked(pp.h, group, _ptr(bytes_d), length, out.ptr, ok.ptr, stream))
    return out, ok.to_numpy(dtype=np.uint8)[:length].copy()
