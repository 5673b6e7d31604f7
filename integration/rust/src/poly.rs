//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_poly.h, the second header of libzkp_pairings.so (symbols added under ABI version 4): the batched
//! NTT over the BLS12-381 scalar field and the KZG opening.  Elements are `[u64; 4]` canonical little-endian limbs (`Fr.0`),
//! points coordinate arrays plus a parallel infinity byte array, as in lib.rs.  Commitment needs no symbol of its own: it is
//! `zkp_g1_msm_batch` with `shared_bases = 1` over the Lagrange setup.
use core::ffi::{c_int, c_uint, c_void};

use crate::ZkpCtx;

/// flags of `zkp_fr_ntt_batch`: evaluations in, coefficients out
pub const ZKP_NTT_INVERSE: c_int = 1;
/// the evaluation side is stored bit-reversed: slot i belongs to w^bitrev(i), as `ZKP_FR_EVAL_BITREV`
pub const ZKP_NTT_BITREV: c_int = 2;
/// the domain is 7 w^i
pub const ZKP_NTT_COSET: c_int = 4;

extern "C" {
    pub fn zkp_fr_ntt_batch(ctx: *mut ZkpCtx, input: *const u64, n_poly: usize, log2_n: c_uint, flags: c_int, out: *mut u64) -> c_int;
    pub fn zkp_fr_ntt_batch_dev(ctx: *mut ZkpCtx, d_in: *const c_void, n_poly: usize, log2_n: c_uint, flags: c_int, d_out: *mut c_void,
                                stream: *mut c_void) -> c_int;
    pub fn zkp_kzg_open_batch(ctx: *mut ZkpCtx, lagrange_g1: *const u64, evals: *const u64, z: *const u64, n: usize, log2_n: c_uint, flags: c_int,
                              out_y: *mut u64, out_proof: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_kzg_open_batch_dev(ctx: *mut ZkpCtx, d_lagrange_g1: *const c_void, d_evals: *const c_void, d_z: *const c_void, n: usize,
                                  log2_n: c_uint, flags: c_int, d_out_y: *mut c_void, d_out_proof: *mut c_void, d_out_inf: *mut c_void,
                                  stream: *mut c_void) -> c_int;
}
