//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_prove.h, the third header of libzkp_pairings.so (symbols added under ABI version 4): the sparse
//! matrix times dense vectors product over the BLS12-381 scalar field, the QAP quotient and the batched Groth16 prover.  Elements
//! are `[u64; 4]` canonical little-endian limbs (`Fr.0`), points coordinate arrays plus a parallel infinity byte array, as in
//! lib.rs.  The descriptors are host structs; their pointers are host pointers for the host flavour and device pointers for the
//! `_dev` one.  The outputs of the prover are laid out as `zkp_groth16_batch`'s a / inf_a / b / inf_b / c / inf_c.
use core::ffi::{c_int, c_uint, c_void};

use crate::ZkpCtx;

/// `zkp_fr_csr`: a sparse matrix in compressed rows; row_ptr: n_rows + 1 u32, col: nnz u32, val: nnz x 4 u64 (canonical)
#[repr(C)]
pub struct ZkpFrCsr {
    pub n_rows: usize,
    pub n_cols: usize,
    pub nnz: usize,
    pub row_ptr: *const c_void,
    pub col: *const c_void,
    pub val: *const c_void,
}

/// `zkp_r1cs`: the three matrices share n_rows and n_cols = m; N = 2^log2_n >= n_rows
#[repr(C)]
pub struct ZkpR1cs {
    pub log2_n: c_uint,
    pub n_inputs: usize,
    pub a: ZkpFrCsr,
    pub b: ZkpFrCsr,
    pub c: ZkpFrCsr,
}

/// `zkp_groth16_pk`: wire-format points, trusted; the four `*_inf` arrays are optional infinity bytes (null: all finite)
#[repr(C)]
pub struct ZkpGroth16Pk {
    pub alpha_g1: *const c_void,
    pub beta_g1: *const c_void,
    pub delta_g1: *const c_void,
    pub beta_g2: *const c_void,
    pub delta_g2: *const c_void,
    pub a_query: *const c_void,
    pub a_inf: *const c_void,
    pub b_g1_query: *const c_void,
    pub b_g1_inf: *const c_void,
    pub b_g2_query: *const c_void,
    pub b_g2_inf: *const c_void,
    pub l_query: *const c_void,
    pub l_inf: *const c_void,
    pub h_query: *const c_void,
}

extern "C" {
    pub fn zkp_fr_spmv_batch(ctx: *mut ZkpCtx, mat: *const ZkpFrCsr, x: *const u64, n: usize, out_stride: usize, out: *mut u64) -> c_int;
    pub fn zkp_fr_spmv_batch_dev(ctx: *mut ZkpCtx, mat: *const ZkpFrCsr, d_x: *const c_void, n: usize, out_stride: usize, d_out: *mut c_void,
                                 stream: *mut c_void) -> c_int;
    pub fn zkp_groth16_quotient_batch(ctx: *mut ZkpCtx, r1cs: *const ZkpR1cs, witness: *const u64, n: usize, out_h: *mut u64, out_sat: *mut u8) -> c_int;
    pub fn zkp_groth16_quotient_batch_dev(ctx: *mut ZkpCtx, r1cs: *const ZkpR1cs, d_witness: *const c_void, n: usize, d_out_h: *mut c_void,
                                          d_out_sat: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_groth16_prove_batch(ctx: *mut ZkpCtx, r1cs: *const ZkpR1cs, pk: *const ZkpGroth16Pk, witness: *const u64, rs: *const u64, n: usize,
                                   flags: c_int, out_a: *mut u64, out_inf_a: *mut u8, out_b: *mut u64, out_inf_b: *mut u8, out_c: *mut u64,
                                   out_inf_c: *mut u8, out_sat: *mut u8) -> c_int;
    pub fn zkp_groth16_prove_batch_dev(ctx: *mut ZkpCtx, r1cs: *const ZkpR1cs, pk: *const ZkpGroth16Pk, d_witness: *const c_void, d_rs: *const c_void,
                                       n: usize, flags: c_int, d_out_a: *mut c_void, d_out_inf_a: *mut c_void, d_out_b: *mut c_void,
                                       d_out_inf_b: *mut c_void, d_out_c: *mut c_void, d_out_inf_c: *mut c_void, d_out_sat: *mut c_void,
                                       stream: *mut c_void) -> c_int;
}
