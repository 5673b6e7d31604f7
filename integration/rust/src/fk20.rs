//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_fk20.h, the fourth header of libzkp_pairings.so (symbols added under ABI version 4): the batched
//! NTT over G1 points and the Feist-Khovratovich KZG proofs of a polynomial at every point of its domain.  Points are coordinate
//! arrays (`[u64; 12]` each) plus a parallel infinity byte array, elements `[u64; 4]` canonical little-endian limbs, as in lib.rs.
//! The flags are `poly::ZKP_NTT_INVERSE` and `poly::ZKP_NTT_BITREV`; there is no coset.
use core::ffi::{c_int, c_uint, c_void};

use crate::ZkpCtx;

extern "C" {
    pub fn zkp_g1_ntt_batch(ctx: *mut ZkpCtx, points: *const u64, inf: *const u8, n_vec: usize, log2_n: c_uint, flags: c_int, out: *mut u64,
                            out_inf: *mut u8) -> c_int;
    pub fn zkp_g1_ntt_batch_dev(ctx: *mut ZkpCtx, d_points: *const c_void, d_inf: *const c_void, n_vec: usize, log2_n: c_uint, flags: c_int,
                                d_out: *mut c_void, d_out_inf: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_kzg_fk20_setup(ctx: *mut ZkpCtx, monomial_g1: *const u64, log2_n: c_uint, out: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_kzg_fk20_setup_dev(ctx: *mut ZkpCtx, d_monomial_g1: *const c_void, log2_n: c_uint, d_out: *mut c_void, d_out_inf: *mut c_void,
                                  stream: *mut c_void) -> c_int;
    pub fn zkp_kzg_fk20_batch(ctx: *mut ZkpCtx, fk20_setup: *const u64, fk20_setup_inf: *const u8, coeffs: *const u64, n: usize, log2_n: c_uint,
                              flags: c_int, out_proof: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_kzg_fk20_batch_dev(ctx: *mut ZkpCtx, d_fk20_setup: *const c_void, d_fk20_setup_inf: *const c_void, d_coeffs: *const c_void, n: usize,
                                  log2_n: c_uint, flags: c_int, d_out_proof: *mut c_void, d_out_inf: *mut c_void, stream: *mut c_void) -> c_int;
}
