//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_recover.h, the sixth header of libzkp_pairings.so (symbols added under ABI version 4): erased blobs back
//! from any half of their cells.  Elements are `[u64; 4]` canonical little-endian limbs, as in lib.rs; `present` holds one byte per
//! cell, `out_ok` one `i32` per blob.  The flag is `poly::ZKP_NTT_BITREV`, the order of the cells and of the values inside a cell.
use core::ffi::{c_int, c_uint, c_void};

use crate::ZkpCtx;

extern "C" {
    pub fn zkp_das_recover_batch(ctx: *mut ZkpCtx, values: *const u64, present: *const u8, n: usize, log2_n: c_uint, log2_l: c_uint, flags: c_int,
                                 out_coeffs: *mut u64, out_ok: *mut i32) -> c_int;
    pub fn zkp_das_recover_batch_dev(ctx: *mut ZkpCtx, d_values: *const c_void, d_present: *const c_void, n: usize, log2_n: c_uint, log2_l: c_uint,
                                     flags: c_int, d_out_coeffs: *mut c_void, d_out_ok: *mut c_void, stream: *mut c_void) -> c_int;
}
