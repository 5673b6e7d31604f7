//! UNTESTED - like the rest of this crate, never compiled (no Rust toolchain in the build image).
//!
//! Raw bindings to include/zkp_bls_agg_g2.h, the eleventh header of libzkp_pairings.so (symbols added under ABI version 4): sums of G2
//! table rows over the segments of a ragged, signed index list (signature aggregation in the min-pk layout, key aggregation in the
//! min-sig layout), FastAggregateVerify for committees of G2 keys, and AggregateVerify (one signature over several (key, message)
//! pairs).  `idx` holds `u32` entries (bit 31: subtract the row), `seg_off` holds one offset more than there are segments; flags are
//! those of bls.rs (`ZKP_BLS_POINTS_CHECKED`).
use core::ffi::{c_int, c_void};

use crate::ZkpCtx;

extern "C" {
    pub fn zkp_g2_segment_sum_batch(ctx: *mut ZkpCtx, table: *const u64, n_table: usize, idx: *const u32, n_idx: usize, seg_off: *const u64,
                                    n_seg: usize, out: *mut u64, out_inf: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_g2_segment_sum_batch_dev(ctx: *mut ZkpCtx, d_table: *const c_void, n_table: usize, d_idx: *const c_void, n_idx: usize,
                                        d_seg_off: *const c_void, n_seg: usize, d_out: *mut c_void, d_out_inf: *mut c_void, d_status: *mut c_void,
                                        stream: *mut c_void) -> c_int;
    pub fn zkp_bls_minsig_fast_aggregate_verify_batch(ctx: *mut ZkpCtx, table: *const u64, n_table: usize, idx: *const u32, n_idx: usize,
                                                      seg_off: *const u64, msgs: *const u8, offsets: *const u64, dst: *const u8, dst_len: usize,
                                                      sig: *const u64, inf_sig: *const u8, n: usize, rand: *const u64, flags: c_int,
                                                      all_ok: *mut c_int) -> c_int;
    pub fn zkp_bls_minsig_fast_aggregate_verify_batch_dev(ctx: *mut ZkpCtx, d_table: *const c_void, n_table: usize, d_idx: *const c_void, n_idx: usize,
                                                          d_seg_off: *const c_void, d_msgs: *const c_void, d_offsets: *const c_void,
                                                          d_dst: *const c_void, dst_len: usize, d_sig: *const c_void, d_inf_sig: *const c_void, n: usize,
                                                          d_rand: *const c_void, flags: c_int, d_all_ok: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn zkp_bls_aggregate_verify_batch(ctx: *mut ZkpCtx, pk: *const u64, inf_pk: *const u8, msgs: *const u8, offsets: *const u64, n_msg: usize,
                                          seg_off: *const u64, dst: *const u8, dst_len: usize, sig: *const u64, inf_sig: *const u8, n: usize,
                                          rand: *const u64, flags: c_int, all_ok: *mut c_int) -> c_int;
    pub fn zkp_bls_aggregate_verify_batch_dev(ctx: *mut ZkpCtx, d_pk: *const c_void, d_inf_pk: *const c_void, d_msgs: *const c_void,
                                              d_offsets: *const c_void, n_msg: usize, d_seg_off: *const c_void, d_dst: *const c_void, dst_len: usize,
                                              d_sig: *const c_void, d_inf_sig: *const c_void, n: usize, d_rand: *const c_void, flags: c_int,
                                              d_all_ok: *mut c_void, stream: *mut c_void) -> c_int;
}
