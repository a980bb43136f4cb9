//! `circuit_specific_setup` in the exponent (`groth16/examples/sha256.rs`, `ark_groth16::generate_parameters` with the
//! circom reduction): R1CS and trapdoor -> the discrete logs of the five CRS vectors, on the device
//! (`zk_groth16_setup_scalars`).  The vectors stay on the device, each followed by `tail_zeros` zero elements, so that
//! `l`-chunked windows go straight to `zk_pss_det_pack` and `zk_base_mul`; `to_vec` brings one back for a test.
use core::ptr;

use ark_ff::PrimeField;
use mpc_net::MpcNetError;
use zksaas_hip_sys as sys;

use crate::{check, fr_ptr, Context, DeviceBuf};

/// One constraint matrix as row-CSR (`ConstraintMatrices::{a, b, c}` flattened): `row_ptr` has one entry per constraint
/// plus one, `col` the wire indices, `val` the coefficients.
pub struct CsrMatrix<'a, F: PrimeField> {
    pub row_ptr: &'a [u32],
    pub col: &'a [u32],
    pub val: &'a [F],
}

/// The discrete logs of `a_query` `[nv]`, `b_query` `[nv]`, `l_query` `[nv - ni]`, `h_query` `[m]` and `gamma_abc` `[ni]`.
pub struct SetupScalars {
    pub a_query: DeviceBuf,
    pub b_query: DeviceBuf,
    pub l_query: DeviceBuf,
    pub h_query: DeviceBuf,
    pub gamma_abc: DeviceBuf,
    pub log_m: u32,
    pub tail_zeros: usize,
}

struct DeviceCsr {
    row_ptr: DeviceBuf,
    col: DeviceBuf,
    val: DeviceBuf,
}

fn upload<F: PrimeField>(ctx: &Context, m: &CsrMatrix<F>, num_constraints: usize) -> Result<DeviceCsr, MpcNetError> {
    if m.row_ptr.len() != num_constraints + 1 || m.col.len() != m.val.len()
        || m.row_ptr[num_constraints] as usize != m.col.len() {
        return Err(MpcNetError::BadInput { err: "setup_scalars: inconsistent CSR arrays" });
    }
    let _ = fr_ptr(m.val);
    Ok(DeviceCsr { row_ptr: DeviceBuf::from_slice(ctx, m.row_ptr)?, col: DeviceBuf::from_slice(ctx, m.col)?,
                   val: DeviceBuf::from_slice(ctx, m.val)? })
}

/// `trapdoor` = alpha, beta, gamma, delta, tau.  The domain is the smallest power of two that holds
/// `num_constraints + num_instance` (`Radix2EvaluationDomain::new`).  A degenerate trapdoor (gamma, delta or tau zero, or
/// tau inside the domain of twice that size) is `BadInput`; a wire index `>= num_variables` is `Generic`.
pub fn setup_scalars<F: PrimeField + 'static>(ctx: &Context, a: &CsrMatrix<F>, b: &CsrMatrix<F>, c: &CsrMatrix<F>,
                                              num_variables: usize, num_instance: usize, trapdoor: &[F; 5],
                                              tail_zeros: usize) -> Result<SetupScalars, MpcNetError> {
    ctx.expect_field::<F>(ctx.l)?;
    if a.row_ptr.is_empty() || num_instance == 0 || num_instance > num_variables {
        return Err(MpcNetError::BadInput { err: "setup_scalars: bad R1CS dimensions" });
    }
    let num_constraints = a.row_ptr.len() - 1;
    let log_m = (num_constraints + num_instance).next_power_of_two().trailing_zeros();
    let (da, db, dc) = (upload(ctx, a, num_constraints)?, upload(ctx, b, num_constraints)?, upload(ctx, c, num_constraints)?);
    let fr = core::mem::size_of::<F>();
    let out = SetupScalars {
        a_query: DeviceBuf::alloc(ctx, (num_variables + tail_zeros) * fr)?,
        b_query: DeviceBuf::alloc(ctx, (num_variables + tail_zeros) * fr)?,
        l_query: DeviceBuf::alloc(ctx, (num_variables - num_instance + tail_zeros) * fr)?,
        h_query: DeviceBuf::alloc(ctx, ((1usize << log_m) + tail_zeros) * fr)?,
        gamma_abc: DeviceBuf::alloc(ctx, num_instance * fr)?,
        log_m,
        tail_zeros,
    };
    check(ctx, unsafe {
        sys::zk_groth16_setup_scalars(ctx.raw(), da.row_ptr.ptr(), da.col.ptr(), da.val.ptr(), db.row_ptr.ptr(), db.col.ptr(),
                                      db.val.ptr(), dc.row_ptr.ptr(), dc.col.ptr(), dc.val.ptr(), num_variables,
                                      num_constraints, num_instance, log_m as i32, fr_ptr(&trapdoor[..]), tail_zeros,
                                      out.a_query.ptr(), out.b_query.ptr(), out.l_query.ptr(), out.h_query.ptr(),
                                      out.gamma_abc.ptr(), ptr::null_mut())
    })?;
    Ok(out)
}
