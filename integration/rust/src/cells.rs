//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_cells.h, the fifth header of libzkp_pairings.so (symbols added under ABI version 4): the KZG cell
//! proofs - Feist-Khovratovich multi-proofs of a polynomial on every coset of l points of its extended domain - and their batch
//! verifier.  Points are coordinate arrays (`[u64; 12]` each, G2 `[u64; 24]`) plus a parallel infinity byte array, elements `[u64; 4]`
//! canonical little-endian limbs, as in lib.rs.  The producer's flag is `poly::ZKP_NTT_BITREV`; the verifier adds the two below.
use core::ffi::{c_int, c_uint, c_void};

use crate::ZkpCtx;

pub const ZKP_CELLS_POINTS_CHECKED: c_int = 4;
pub const ZKP_CELLS_VK_CHECKED: c_int = 8;

extern "C" {
    pub fn zkp_kzg_cells_setup(ctx: *mut ZkpCtx, monomial_g1: *const u64, log2_n: c_uint, log2_l: c_uint, out: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_kzg_cells_setup_dev(ctx: *mut ZkpCtx, d_monomial_g1: *const c_void, log2_n: c_uint, log2_l: c_uint, d_out: *mut c_void,
                                   d_out_inf: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_kzg_cells_batch(ctx: *mut ZkpCtx, cells_setup: *const u64, cells_setup_inf: *const u8, coeffs: *const u64, n: usize, log2_n: c_uint,
                               log2_l: c_uint, log2_ext: c_uint, flags: c_int, out_proof: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_kzg_cells_batch_dev(ctx: *mut ZkpCtx, d_cells_setup: *const c_void, d_cells_setup_inf: *const c_void, d_coeffs: *const c_void, n: usize,
                                   log2_n: c_uint, log2_l: c_uint, log2_ext: c_uint, flags: c_int, d_out_proof: *mut c_void, d_out_inf: *mut c_void,
                                   stream: *mut c_void) -> c_int;
    pub fn zkp_kzg_cell_verify_batch(ctx: *mut ZkpCtx, monomial_g1_l: *const u64, g2: *const u64, tau_l_g2: *const u64, commitments: *const u64,
                                     inf_c: *const u8, cell_index: *const u32, values: *const u64, proofs: *const u64, inf_proof: *const u8, n: usize,
                                     log2_d: c_uint, log2_l: c_uint, flags: c_int, rand: *const u64, out_ok: *mut c_int) -> c_int;
    pub fn zkp_kzg_cell_verify_batch_dev(ctx: *mut ZkpCtx, d_monomial_g1_l: *const c_void, d_g2: *const c_void, d_tau_l_g2: *const c_void,
                                         d_commitments: *const c_void, d_inf_c: *const c_void, d_cell_index: *const c_void, d_values: *const c_void,
                                         d_proofs: *const c_void, d_inf_proof: *const c_void, n: usize, log2_d: c_uint, log2_l: c_uint, flags: c_int,
                                         d_rand: *const c_void, d_out_ok: *mut c_void, stream: *mut c_void) -> c_int;
}
