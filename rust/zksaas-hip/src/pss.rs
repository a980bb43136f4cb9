//! `PackedSharingParams` batch methods on the GPU (`secret-sharing/src/pss.rs:69-221`,
//! `dist-primitives/src/utils/pack.rs:8-35`).  The reference packs one chunk per call and transposes `Vec<Vec<F>>`;
//! here a whole vector is packed / unpacked per launch and the party-major layout `[n][m/l]` needs no transpose.
use core::ptr;

use ark_ec::short_weierstrass::{Affine, SWCurveConfig};
use ark_ff::PrimeField;
use mpc_net::MpcNetError;
use zksaas_hip_sys as sys;

use crate::{check, fr_ptr, group_of, pack_affine, unpack_affine, Context, DeviceBuf};

/// `pack_vec` + `transpose` (`pack.rs:8-35`): secrets `[m]` -> `n` share vectors of length `m / l`.
pub fn pack_vec<F: PrimeField + 'static>(ctx: &Context, secrets: &[F]) -> Result<Vec<Vec<F>>, MpcNetError> {
    pack_impl(ctx, secrets, 0, false)
}
/// Stride packing (`dfft/mod.rs:286-299`, `qap.rs:103-112`): chunk `j` packs `secrets[j], secrets[j + m/l], ..`.
pub fn pack_stride<F: PrimeField + 'static>(ctx: &Context, secrets: &[F]) -> Result<Vec<Vec<F>>, MpcNetError> {
    pack_impl(ctx, secrets, 1, false)
}
/// `det_pack` per chunk (`pss.rs:69-87`).
pub fn det_pack_vec<F: PrimeField + 'static>(ctx: &Context, secrets: &[F]) -> Result<Vec<Vec<F>>, MpcNetError> {
    pack_impl(ctx, secrets, 0, true)
}

fn pack_impl<F: PrimeField + 'static>(ctx: &Context, secrets: &[F], order: i32, det: bool)
                                      -> Result<Vec<Vec<F>>, MpcNetError> {
    if secrets.len() % ctx.l != 0 {
        return Err(MpcNetError::BadInput { err: "pack: length is not a multiple of l" });
    }
    let nchunks = secrets.len() / ctx.l;
    let sec = DeviceBuf::from_slice(ctx, secrets)?;
    let sh = DeviceBuf::alloc(ctx, ctx.n * nchunks * core::mem::size_of::<F>())?;
    let rc = unsafe {
        if det {
            sys::zk_pss_det_pack(ctx.raw(), sec.ptr(), nchunks, order, sh.ptr(), ptr::null_mut())
        } else {
            sys::zk_pss_pack(ctx.raw(), sec.ptr(), nchunks, order, 0, sh.ptr(), ptr::null_mut())
        }
    };
    check(ctx, rc)?;
    let flat: Vec<F> = sh.to_vec(ctx.n * nchunks)?;
    Ok(flat.chunks(nchunks.max(1)).map(|c| c.to_vec()).collect())
}

/// `unpack` of every chunk (`pss.rs:125-138`): shares `[n][m/l]` -> secrets `[m]` in `pack_vec` order.
pub fn unpack_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>]) -> Result<Vec<F>, MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, ctx.n)?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let out = DeviceBuf::alloc(ctx, nchunks * ctx.l * core::mem::size_of::<F>())?;
    check(ctx, unsafe { sys::zk_pss_unpack(ctx.raw(), sh.ptr(), nchunks, out.ptr(), ptr::null_mut()) })?;
    out.to_vec(nchunks * ctx.l)
}

/// `unpack_missing_shares` of every chunk (`pss.rs:210-221`): `unpack2` when all `n` parties are present, the
/// Lagrange form (`:170-205`) for the listed subset otherwise.
pub fn unpack_missing_shares_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32])
                                                          -> Result<Vec<F>, MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, parties.len())?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let out = DeviceBuf::alloc(ctx, nchunks * ctx.l * core::mem::size_of::<F>())?;
    check(ctx, unsafe {
        sys::zk_pss_unpack2(ctx.raw(), sh.ptr(), parties.as_ptr(), parties.len() as i32, nchunks, out.ptr(),
                            ptr::null_mut())
    })?;
    out.to_vec(nchunks * ctx.l)
}

/// Verdict of [`unpack_robust_vec`] / [`unpack_robust_parties_vec`] for one chunk.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Verdict {
    /// the interpolant of the (listed) shares already has degree `< dimension`
    Clean,
    /// up to `(n - dimension) / 2` shares (`n`: the number of listed parties) were wrong and have been corrected; `errpos` names the parties
    Corrected,
    /// no polynomial of degree `< dimension` lies that close: secrets and message read as zero
    Failed,
}

/// What [`unpack_robust_vec`] returns: `decode_to_message`'s message and the secrets of every chunk, with a verdict
/// in place of its panic.
pub struct RobustUnpack<F> {
    /// `[m]` in `pack_vec` order (zeros for a failed chunk)
    pub secrets: Vec<F>,
    /// coefficient `j` of chunk `c`'s message polynomial at `[j][c]`, `j < dimension`
    pub message: Vec<Vec<F>>,
    pub verdicts: Vec<Verdict>,
    /// bit `p` set: party `p`'s share of the chunk was corrected
    pub errpos: Vec<u32>,
    /// chunks clean, corrected, failed
    pub counts: [u64; 3],
    /// per party, the number of chunks in which its share was corrected
    pub corrected_per_party: Vec<u64>,
}

/// The role of `decode_to_message` (`secret-sharing/src/gao.rs:47-84`) for every chunk of a vector at once, with the
/// early return for a codeword and the checks for a failed decoding its todo lines ask for: `shares` are all `n`
/// parties' vectors, `dimension` is `2l` for packed shares and `4l - 1` for their products.  Bad shares never make
/// the call fail; they show in the verdicts.  With parties absent the call is [`unpack_robust_parties_vec`].
pub fn unpack_robust_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], dimension: usize)
                                                  -> Result<RobustUnpack<F>, MpcNetError> {
    robust_impl(ctx, shares, None, dimension)
}

/// [`unpack_robust_vec`] for the share vectors of the listed parties only (ascending ids, the list of
/// `unpack_missing_shares`, `secret-sharing/src/pss.rs:141-221`): dropouts and wrong shares in one chunk.  Up to
/// `(parties.len() - dimension) / 2` wrong shares among the listed are corrected per chunk; `errpos` and
/// `corrected_per_party` stay indexed by party id and never name an absent party.  A party named once can be left out
/// of the list afterwards.  `parties.len() <= dimension` is `MpcNetError::Protocol`, as for `unpack_missing_shares`.
pub fn unpack_robust_parties_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32],
                                                          dimension: usize) -> Result<RobustUnpack<F>, MpcNetError> {
    robust_impl(ctx, shares, Some(parties), dimension)
}

fn robust_impl<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: Option<&[u32]>, dimension: usize)
                                        -> Result<RobustUnpack<F>, MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, parties.map_or(ctx.n, |p| p.len()))?;
    let fsz = core::mem::size_of::<F>();
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let sec = DeviceBuf::alloc(ctx, nchunks * ctx.l * fsz)?;
    let msg = DeviceBuf::alloc(ctx, nchunks * dimension * fsz)?;
    let st = DeviceBuf::alloc(ctx, nchunks)?;
    let ep = DeviceBuf::alloc(ctx, nchunks * 4)?;
    let sm = DeviceBuf::alloc(ctx, (3 + ctx.n) * 8)?;
    check(ctx, unsafe {
        match parties {
            None => sys::zk_pss_unpack_robust(ctx.raw(), sh.ptr(), nchunks, dimension as i32, sec.ptr(), msg.ptr(),
                                              st.ptr() as *mut u8, ep.ptr() as *mut u32, sm.ptr() as *mut u64, ptr::null_mut()),
            Some(p) => sys::zk_pss_unpack_robust_parties(ctx.raw(), sh.ptr(), p.as_ptr(), p.len() as i32, nchunks,
                                                         dimension as i32, sec.ptr(), msg.ptr(), st.ptr() as *mut u8,
                                                         ep.ptr() as *mut u32, sm.ptr() as *mut u64, ptr::null_mut()),
        }
    })?;
    let status: Vec<u8> = st.to_vec(nchunks)?;
    let summary: Vec<u64> = if nchunks == 0 { vec![0; 3 + ctx.n] } else { sm.to_vec(3 + ctx.n)? };
    let message: Vec<F> = msg.to_vec(nchunks * dimension)?;
    Ok(RobustUnpack {
        secrets: sec.to_vec(nchunks * ctx.l)?,
        message: message.chunks(nchunks.max(1)).map(|c| c.to_vec()).collect(),
        verdicts: status.iter().map(|s| match s { 0 => Verdict::Clean, 1 => Verdict::Corrected, _ => Verdict::Failed }).collect(),
        errpos: ep.to_vec(nchunks)?,
        counts: [summary[0], summary[1], summary[2]],
        corrected_per_party: summary[3..].to_vec(),
    })
}

/// The verdicts of [`repair_vec`] and of the checked king rounds: [`RobustUnpack`] without secrets and message.
pub struct Verdicts {
    pub verdicts: Vec<Verdict>,
    /// bit `p` set: party `p`'s share of the chunk was wrong and has been replaced
    pub errpos: Vec<u32>,
    /// chunks clean, corrected, failed
    pub counts: [u64; 3],
    /// per party, the number of chunks in which its share was corrected
    pub corrected_per_party: Vec<u64>,
}

struct VerdictBufs {
    st: DeviceBuf,
    ep: DeviceBuf,
    sm: DeviceBuf,
    nchunks: usize,
}
impl VerdictBufs {
    fn alloc(ctx: &Context, nchunks: usize) -> Result<Self, MpcNetError> {
        Ok(VerdictBufs { st: DeviceBuf::alloc(ctx, nchunks)?, ep: DeviceBuf::alloc(ctx, nchunks * 4)?,
                         sm: DeviceBuf::alloc(ctx, (3 + ctx.n) * 8)?, nchunks })
    }
    fn read(&self, ctx: &Context) -> Result<Verdicts, MpcNetError> {
        let status: Vec<u8> = self.st.to_vec(self.nchunks)?;
        let summary: Vec<u64> = if self.nchunks == 0 { vec![0; 3 + ctx.n] } else { self.sm.to_vec(3 + ctx.n)? };
        Ok(Verdicts {
            verdicts: status.iter().map(|s| match s { 0 => Verdict::Clean, 1 => Verdict::Corrected, _ => Verdict::Failed }).collect(),
            errpos: self.ep.to_vec(self.nchunks)?,
            counts: [summary[0], summary[1], summary[2]],
            corrected_per_party: summary[3..].to_vec(),
        })
    }
}

fn rows<F: PrimeField>(buf: &DeviceBuf, n: usize, len: usize) -> Result<Vec<Vec<F>>, MpcNetError> {
    let flat: Vec<F> = buf.to_vec(n * len)?;
    Ok(flat.chunks(len.max(1)).map(|c| c.to_vec()).collect())
}

/// `zk_pss_repair`: the verdicts of [`unpack_robust_vec`] written back into the shares -- `decode_to_message`
/// (`secret-sharing/src/gao.rs:47-84`) per chunk, then the share of every party named in `errpos` replaced by the
/// decoded polynomial's value.  Every other share is returned as it came: clean chunks, failed chunks, the right shares
/// of a corrected chunk.  All `n` parties.
pub fn repair_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], dimension: usize)
                                           -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, ctx.n)?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        sys::zk_pss_repair(ctx.raw(), sh.ptr(), nchunks, dimension as i32, v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32,
                           v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    Ok((rows(&sh, ctx.n, nchunks)?, v.read(ctx)?))
}

/// The king of `d_fft` / `d_ifft` (`dist-primitives/src/dfft/mod.rs:264-304`) on all `n` parties' vectors after
/// `fft1_in_place`, with the received word repaired first (`zk_fft2_king_checked`; dimension `2l`: up to `l` wrong
/// shares per chunk).  Returns the parties' output shares, the repaired input and the verdicts per input chunk.  A failed
/// chunk is no error: its shares reach the king as received, `counts[2]` says how many.
#[allow(clippy::too_many_arguments)]
pub fn fft2_king_checked_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], log2_m: u32, inverse: bool, g: F,
                                                      scale_size_inv: bool, rearrange: bool, out_mask: Option<&[F]>)
                                                      -> Result<(Vec<Vec<F>>, Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, ctx.n)?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let out = DeviceBuf::alloc(ctx, flat.len() * core::mem::size_of::<F>())?;
    let om = match out_mask { Some(m) => Some(DeviceBuf::from_slice(ctx, m)?), None => None };
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    let gl = [g];
    check(ctx, unsafe {
        sys::zk_fft2_king_checked(ctx.raw(), sh.ptr(), ptr::null(), ctx.n as i32, log2_m as i32, inverse as i32, fr_ptr(&gl),
                                  scale_size_inv as i32, rearrange as i32, 0, out.ptr(),
                                  om.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void),
                                  v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    Ok((rows(&out, ctx.n, nchunks)?, rows(&sh, ctx.n, nchunks)?, v.read(ctx)?))
}

/// `d_fft` (`dfft/mod.rs:99-134`) for all `n` parties on this device with the king's word `fft1(x) + in_mask` repaired
/// first (`zk_d_fft_checked`): a party whose whole vector is wrong -- and up to `l` of them -- is named in the verdicts
/// and the output is the honest one.  `in_mask` / `out_mask`: all parties' masks `[n][m/l]` flattened, or `None`.
pub fn d_fft_checked_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], in_mask: Option<&[F]>,
                                                  out_mask: Option<&[F]>, rearrange: bool, log2_m: u32)
                                                  -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    transform_checked(ctx, shares, in_mask, out_mask, rearrange, log2_m, None)
}

/// `d_ifft` (`dfft/mod.rs:137-175`) in the same way (`zk_d_ifft_checked`): the word is `fft1(x) / m + in_mask` (`:159`).
pub fn d_ifft_checked_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], in_mask: Option<&[F]>,
                                                   out_mask: Option<&[F]>, rearrange: bool, log2_m: u32, g: F)
                                                   -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    transform_checked(ctx, shares, in_mask, out_mask, rearrange, log2_m, Some(g))
}

fn transform_checked<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], in_mask: Option<&[F]>,
                                              out_mask: Option<&[F]>, rearrange: bool, log2_m: u32, g: Option<F>)
                                              -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, ctx.n)?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let up = |m: Option<&[F]>| -> Result<Option<DeviceBuf>, MpcNetError> {
        match m {
            Some(m) if m.len() != flat.len() => Err(MpcNetError::BadInput { err: "FftMask length differs from the share vectors" }),
            Some(m) => Ok(Some(DeviceBuf::from_slice(ctx, m)?)),
            None => Ok(None),
        }
    };
    let (im, om) = (up(in_mask)?, up(out_mask)?);
    let p = |b: &Option<DeviceBuf>| b.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void);
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        match g {
            None => sys::zk_d_fft_checked(ctx.raw(), sh.ptr(), p(&im), p(&om), rearrange as i32, log2_m as i32, 0,
                                          ptr::null_mut(), v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32,
                                          v.sm.ptr() as *mut u64, ptr::null_mut()),
            Some(g) => {
                let gl = [g];
                sys::zk_d_ifft_checked(ctx.raw(), sh.ptr(), p(&im), p(&om), rearrange as i32, log2_m as i32, fr_ptr(&gl), 0,
                                       ptr::null_mut(), v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32,
                                       v.sm.ptr() as *mut u64, ptr::null_mut())
            }
        }
    })?;
    Ok((rows(&sh, ctx.n, nchunks)?, v.read(ctx)?))
}

/// `deg_red` (`dist-primitives/src/utils/deg_red.rs:99-115`) for all `n` parties on this device with the king's word
/// `x + in_mask` checked (`zk_deg_red_checked`).  The word has dimension `4l - 1`, which leaves no redundancy to correct
/// with (`gao.rs`: cap `(n - k) / 2 = 0`): DETECTION ONLY.  A verdict is `Clean` or `Failed`, and the output is
/// `deg_red`'s on the same input.
pub fn deg_red_checked_vec<F: PrimeField + 'static>(ctx: &Context, x_shares: &[Vec<F>], in_mask: Option<&[F]>,
                                                    out_mask: Option<&[F]>)
                                                    -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, len) = flatten(ctx, x_shares, ctx.n)?;
    let x = DeviceBuf::from_slice(ctx, &flat)?;
    let up = |m: Option<&[F]>| -> Result<Option<DeviceBuf>, MpcNetError> {
        match m {
            Some(m) if m.len() != flat.len() => Err(MpcNetError::BadInput { err: "DegRedMask length differs from the share vectors" }),
            Some(m) => Ok(Some(DeviceBuf::from_slice(ctx, m)?)),
            None => Ok(None),
        }
    };
    let (im, om) = (up(in_mask)?, up(out_mask)?);
    let p = |b: &Option<DeviceBuf>| b.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void);
    let v = VerdictBufs::alloc(ctx, len)?;
    check(ctx, unsafe {
        sys::zk_deg_red_checked(ctx.raw(), x.ptr(), p(&im), p(&om), len, 0, v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32,
                                v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    Ok((rows(&x, ctx.n, len)?, v.read(ctx)?))
}

/// `zk_pss_repair_parties`: [`repair_vec`] for the share vectors of the listed parties only (ascending ids, the list of
/// `unpack_missing_shares`, `secret-sharing/src/pss.rs:141-221`).  The verdicts are [`unpack_robust_parties_vec`]'s; in a
/// corrected chunk the share of every listed party named in `errpos` -- by party id -- is replaced in that party's row.
/// An absent party has no row and its share is not recovered.  `parties.len() <= dimension` is `MpcNetError::Protocol`.
pub fn repair_parties_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32], dimension: usize)
                                                   -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, parties.len())?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        sys::zk_pss_repair_parties(ctx.raw(), sh.ptr(), parties.as_ptr(), parties.len() as i32, nchunks, dimension as i32,
                                   v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    Ok((rows(&sh, parties.len(), nchunks)?, v.read(ctx)?))
}

/// `zk_pss_unpack_points_robust`: the robust unpack of all `n` parties' packed POINT shares, one vector of affine points per
/// party (`secret-sharing/src/pss.rs:125-166` with `T` a group element).  One wrong share per chunk is located and corrected
/// when `n - dimension >= 2`; at dimension `4l - 1` the call only detects.  Returns `[nchunks][l]` points -- the unpack of the
/// clean or corrected word, the identity for a failed chunk -- and the verdicts.
pub fn unpack_points_robust_vec<C: SWCurveConfig>(ctx: &Context, shares: &[Vec<Affine<C>>], dimension: usize)
                                                  -> Result<(Vec<Affine<C>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten_points::<C>(shares, ctx.n)?;
    let limbs = pack_affine(&flat);
    let per = if flat.is_empty() { 0 } else { limbs.len() / flat.len() };
    let sh = DeviceBuf::from_slice(ctx, &limbs)?;
    let out = DeviceBuf::alloc(ctx, nchunks * ctx.l * per * 8)?;
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        sys::zk_pss_unpack_points_robust(ctx.raw(), group_of::<C>(), sh.ptr(), nchunks, dimension as i32, out.ptr(),
                                         v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    let got: Vec<u64> = out.to_vec(nchunks * ctx.l * per)?;
    Ok((unpack_affine::<C>(&got, nchunks * ctx.l), v.read(ctx)?))
}

/// `zk_pss_repair_points`: the verdicts of [`unpack_points_robust_vec`] written back into the shares: in a corrected chunk
/// the one share `errpos` names is replaced by the honest one, every other point is returned as it came.
pub fn repair_points_vec<C: SWCurveConfig>(ctx: &Context, shares: &[Vec<Affine<C>>], dimension: usize)
                                           -> Result<(Vec<Vec<Affine<C>>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten_points::<C>(shares, ctx.n)?;
    let limbs = pack_affine(&flat);
    let sh = DeviceBuf::from_slice(ctx, &limbs)?;
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        sys::zk_pss_repair_points(ctx.raw(), group_of::<C>(), sh.ptr(), nchunks, dimension as i32, v.st.ptr() as *mut u8,
                                  v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64, ptr::null_mut())
    })?;
    let got: Vec<u64> = sh.to_vec(limbs.len())?;
    let pts = unpack_affine::<C>(&got, flat.len());
    Ok((pts.chunks(nchunks.max(1)).map(|c| c.to_vec()).collect(), v.read(ctx)?))
}

fn flatten_points<C: SWCurveConfig>(shares: &[Vec<Affine<C>>], want: usize) -> Result<(Vec<Affine<C>>, usize), MpcNetError> {
    if shares.len() != want || shares.iter().any(|r| r.len() != shares[0].len()) {
        return Err(MpcNetError::BadInput { err: "one vector of equal length per party expected" });
    }
    Ok((shares.iter().flat_map(|r| r.iter().copied()).collect(), shares[0].len()))
}

/// [`fft2_king_checked_vec`] when only the listed parties' vectors reached the king (`zk_fft2_king_checked_parties`):
/// `shares` holds one vector per listed party; up to `(parties.len() - 2l) / 2` wrong shares per chunk are corrected.
/// Returns the `n` parties' output shares, the repaired input rows and the verdicts per input chunk.
#[allow(clippy::too_many_arguments)]
pub fn fft2_king_checked_parties_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32], log2_m: u32,
                                                              inverse: bool, g: F, scale_size_inv: bool, rearrange: bool,
                                                              out_mask: Option<&[F]>)
                                                              -> Result<(Vec<Vec<F>>, Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, parties.len())?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let out = DeviceBuf::alloc(ctx, ctx.n * nchunks * core::mem::size_of::<F>())?;
    let om = match out_mask { Some(m) => Some(DeviceBuf::from_slice(ctx, m)?), None => None };
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    let gl = [g];
    check(ctx, unsafe {
        sys::zk_fft2_king_checked_parties(ctx.raw(), sh.ptr(), parties.as_ptr(), parties.len() as i32, log2_m as i32,
                                          inverse as i32, fr_ptr(&gl), scale_size_inv as i32, rearrange as i32, 0, out.ptr(),
                                          om.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void),
                                          v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64,
                                          ptr::null_mut())
    })?;
    Ok((rows(&out, ctx.n, nchunks)?, rows(&sh, parties.len(), nchunks)?, v.read(ctx)?))
}

/// [`d_fft_checked_vec`] when only the listed parties' words reach the king (`zk_d_fft_checked_parties`).  `shares` and
/// the masks stay `[n][m/l]`; the rows of absent parties are never read.  A party named in an earlier report can be left
/// out of the list: its chunks are clean again and none reaches the decoder.
pub fn d_fft_checked_parties_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32],
                                                          in_mask: Option<&[F]>, out_mask: Option<&[F]>, rearrange: bool,
                                                          log2_m: u32) -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    transform_checked_parties(ctx, shares, parties, in_mask, out_mask, rearrange, log2_m, None)
}

/// `d_ifft` in the same way (`zk_d_ifft_checked_parties`).
#[allow(clippy::too_many_arguments)]
pub fn d_ifft_checked_parties_vec<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32],
                                                           in_mask: Option<&[F]>, out_mask: Option<&[F]>, rearrange: bool,
                                                           log2_m: u32, g: F) -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    transform_checked_parties(ctx, shares, parties, in_mask, out_mask, rearrange, log2_m, Some(g))
}

#[allow(clippy::too_many_arguments)]
fn transform_checked_parties<F: PrimeField + 'static>(ctx: &Context, shares: &[Vec<F>], parties: &[u32], in_mask: Option<&[F]>,
                                                      out_mask: Option<&[F]>, rearrange: bool, log2_m: u32, g: Option<F>)
                                                      -> Result<(Vec<Vec<F>>, Verdicts), MpcNetError> {
    let (flat, nchunks) = flatten(ctx, shares, ctx.n)?;
    let sh = DeviceBuf::from_slice(ctx, &flat)?;
    let up = |m: Option<&[F]>| -> Result<Option<DeviceBuf>, MpcNetError> {
        match m {
            Some(m) if m.len() != flat.len() => Err(MpcNetError::BadInput { err: "FftMask length differs from the share vectors" }),
            Some(m) => Ok(Some(DeviceBuf::from_slice(ctx, m)?)),
            None => Ok(None),
        }
    };
    let (im, om) = (up(in_mask)?, up(out_mask)?);
    let p = |b: &Option<DeviceBuf>| b.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void);
    let v = VerdictBufs::alloc(ctx, nchunks)?;
    check(ctx, unsafe {
        match g {
            None => sys::zk_d_fft_checked_parties(ctx.raw(), sh.ptr(), parties.as_ptr(), parties.len() as i32, p(&im), p(&om),
                                                  rearrange as i32, log2_m as i32, 0, ptr::null_mut(), v.st.ptr() as *mut u8,
                                                  v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64, ptr::null_mut()),
            Some(g) => {
                let gl = [g];
                sys::zk_d_ifft_checked_parties(ctx.raw(), sh.ptr(), parties.as_ptr(), parties.len() as i32, p(&im), p(&om),
                                               rearrange as i32, log2_m as i32, fr_ptr(&gl), 0, ptr::null_mut(),
                                               v.st.ptr() as *mut u8, v.ep.ptr() as *mut u32, v.sm.ptr() as *mut u64,
                                               ptr::null_mut())
            }
        }
    })?;
    Ok((rows(&sh, ctx.n, nchunks)?, v.read(ctx)?))
}

/// `d_pp` (`dist-primitives/src/dpp/mod.rs:15-87`) with the king's word `num ++ den` (`:37-52`) repaired first
/// (`zk_d_pp_checked`): packed shares of degree below `2l`, so up to `(parties.len() - 2l) / 2` wrong shares per chunk are
/// corrected in each half.  `num` and `den` hold one vector per listed party (`None`: all `n`).  Returns the `n` parties'
/// output shares and the verdicts of `num`'s and of `den`'s chunks.  The `deg_red` that ends `d_pp` is not checked.
#[allow(clippy::type_complexity)]
pub fn d_pp_checked_vec<F: PrimeField + 'static>(ctx: &Context, num: &[Vec<F>], den: &[Vec<F>], parties: Option<&[u32]>,
                                                 in_mask: Option<&[F]>, out_mask: Option<&[F]>)
                                                 -> Result<(Vec<Vec<F>>, Verdicts, Verdicts), MpcNetError> {
    let np = parties.map_or(ctx.n, |p| p.len());
    let (nflat, len) = flatten(ctx, num, np)?;
    let (dflat, dlen) = flatten(ctx, den, np)?;
    if dlen != len {
        return Err(MpcNetError::BadInput { err: "d_pp: num and den differ in length" });
    }
    let (nd, dd) = (DeviceBuf::from_slice(ctx, &nflat)?, DeviceBuf::from_slice(ctx, &dflat)?);
    let up = |m: Option<&[F]>| -> Result<Option<DeviceBuf>, MpcNetError> {
        match m {
            Some(m) if m.len() != ctx.n * len => Err(MpcNetError::BadInput { err: "DegRedMask length differs from the share vectors" }),
            Some(m) => Ok(Some(DeviceBuf::from_slice(ctx, m)?)),
            None => Ok(None),
        }
    };
    let (im, om) = (up(in_mask)?, up(out_mask)?);
    let p = |b: &Option<DeviceBuf>| b.as_ref().map_or(ptr::null(), |b| b.ptr() as *const core::ffi::c_void);
    let out = DeviceBuf::alloc(ctx, ctx.n * len * core::mem::size_of::<F>())?;
    let w = 3 + ctx.n;
    let (st, ep, sm) = (DeviceBuf::alloc(ctx, 2 * len)?, DeviceBuf::alloc(ctx, 2 * len * 4)?, DeviceBuf::alloc(ctx, 2 * w * 8)?);
    check(ctx, unsafe {
        sys::zk_d_pp_checked(ctx.raw(), nd.ptr(), dd.ptr(), parties.map_or(ptr::null(), |p| p.as_ptr()), np as i32, p(&im),
                             p(&om), len, 0, out.ptr(), st.ptr() as *mut u8, ep.ptr() as *mut u32, sm.ptr() as *mut u64,
                             ptr::null_mut())
    })?;
    let status: Vec<u8> = st.to_vec(2 * len)?;
    let errpos: Vec<u32> = ep.to_vec(2 * len)?;
    let summary: Vec<u64> = if len == 0 { vec![0; 2 * w] } else { sm.to_vec(2 * w)? };
    let half = |i: usize| Verdicts {
        verdicts: status[i * len..(i + 1) * len].iter()
            .map(|s| match s { 0 => Verdict::Clean, 1 => Verdict::Corrected, _ => Verdict::Failed }).collect(),
        errpos: errpos[i * len..(i + 1) * len].to_vec(),
        counts: [summary[i * w], summary[i * w + 1], summary[i * w + 2]],
        corrected_per_party: summary[i * w + 3..(i + 1) * w].to_vec(),
    };
    Ok((rows(&out, ctx.n, len)?, half(0), half(1)))
}

fn flatten<F: PrimeField>(_ctx: &Context, shares: &[Vec<F>], want: usize) -> Result<(Vec<F>, usize), MpcNetError> {
    if shares.len() != want || shares.is_empty() {
        return Err(MpcNetError::BadInput { err: "unpack: one share vector per listed party expected" });
    }
    let nchunks = shares[0].len();
    if shares.iter().any(|v| v.len() != nchunks) {
        return Err(MpcNetError::BadInput { err: "unpack: share vectors differ in length" });
    }
    let mut flat = Vec::with_capacity(want * nchunks);
    for v in shares {
        flat.extend_from_slice(v);
    }
    let _ = fr_ptr(&flat);
    Ok((flat, nchunks))
}
