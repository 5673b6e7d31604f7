//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_bls_minsig.h, the tenth header of libzkp_pairings.so (symbols added under ABI version 4): messages hashed
//! to G1 (RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_) and the minimal-signature-size BLS batch verifiers, signatures in G1 and public keys
//! in G2.  Field elements are `[u64; 6]` canonical little-endian limbs, as in lib.rs; messages are one byte buffer plus `n + 1` offsets;
//! `all_ok` is one `c_int`; the flag is `bls::ZKP_BLS_POINTS_CHECKED`.
use core::ffi::{c_int, c_void};

use crate::ZkpCtx;

extern "C" {
    pub fn zkp_hash_to_field_g1_batch(ctx: *mut ZkpCtx, msgs: *const u8, offsets: *const u64, n: usize, dst: *const u8, dst_len: usize,
                                      out_u: *mut u64) -> c_int;
    pub fn zkp_hash_to_field_g1_batch_dev(ctx: *mut ZkpCtx, d_msgs: *const c_void, d_offsets: *const c_void, n: usize, d_dst: *const c_void, dst_len: usize,
                                          d_out_u: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_g1_map_from_fields_batch(ctx: *mut ZkpCtx, u: *const u64, n: usize, out: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_g1_map_from_fields_batch_dev(ctx: *mut ZkpCtx, d_u: *const c_void, n: usize, d_out: *mut c_void, d_out_inf: *mut c_void,
                                            stream: *mut c_void) -> c_int;
    pub fn zkp_g1_clear_cofactor_batch(ctx: *mut ZkpCtx, pts: *const u64, inf: *const u8, n: usize, out: *mut u64, out_inf: *mut u8) -> c_int;
    pub fn zkp_g1_clear_cofactor_batch_dev(ctx: *mut ZkpCtx, d_pts: *const c_void, d_inf: *const c_void, n: usize, d_out: *mut c_void,
                                           d_out_inf: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_hash_to_g1_batch(ctx: *mut ZkpCtx, msgs: *const u8, offsets: *const u64, n: usize, dst: *const u8, dst_len: usize, out: *mut u64,
                                out_inf: *mut u8) -> c_int;
    pub fn zkp_hash_to_g1_batch_dev(ctx: *mut ZkpCtx, d_msgs: *const c_void, d_offsets: *const c_void, n: usize, d_dst: *const c_void, dst_len: usize,
                                    d_out: *mut c_void, d_out_inf: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_bls_minsig_verify_batch(ctx: *mut ZkpCtx, pk: *const u64, inf_pk: *const u8, msgs: *const u8, offsets: *const u64, dst: *const u8,
                                       dst_len: usize, sig: *const u64, inf_sig: *const u8, n: usize, rand: *const u64, flags: c_int,
                                       all_ok: *mut c_int) -> c_int;
    pub fn zkp_bls_minsig_verify_batch_dev(ctx: *mut ZkpCtx, d_pk: *const c_void, d_inf_pk: *const c_void, d_msgs: *const c_void, d_offsets: *const c_void,
                                           d_dst: *const c_void, dst_len: usize, d_sig: *const c_void, d_inf_sig: *const c_void, n: usize,
                                           d_rand: *const c_void, flags: c_int, d_all_ok: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_bls_minsig_verify_samekey_batch(ctx: *mut ZkpCtx, pk: *const u64, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                                               sig: *const u64, inf_sig: *const u8, n: usize, rand: *const u64, flags: c_int,
                                               all_ok: *mut c_int) -> c_int;
    pub fn zkp_bls_minsig_verify_samekey_batch_dev(ctx: *mut ZkpCtx, d_pk: *const c_void, d_msgs: *const c_void, d_offsets: *const c_void,
                                                   d_dst: *const c_void, dst_len: usize, d_sig: *const c_void, d_inf_sig: *const c_void, n: usize,
                                                   d_rand: *const c_void, flags: c_int, d_all_ok: *mut c_void, stream: *mut c_void) -> c_int;
}
