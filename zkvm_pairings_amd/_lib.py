"""ctypes loader for libzkp_pairings.so (the C ABI declared in include/zkp_pairings.h, include/zkp_poly.h and include/zkp_prove.h).

No fallback of any kind: if the library is missing or a GPU is not usable the import / call
raises.  The product never imports anything under oracle/."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZKP_LIB_PATH: A/B timing of two builds of the same library on one GPU box (development only)
LIB_PATH = os.environ.get("ZKP_LIB_PATH") or os.path.join(_HERE, "libzkp_pairings.so")

c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_vp = ctypes.c_void_p
c_sz = ctypes.c_size_t
c_int = ctypes.c_int

RLC_POINTS_CHECKED = 1   # ZKP_RLC_POINTS_CHECKED


class RlcBatch(ctypes.Structure):
    """zkp_rlc_batch: the shape of a batch for zkp_pairing_check_batch_rlc[_dev] (field order of include/zkp_pairings.h)"""
    _fields_ = [("n_checks", c_sz),
                ("k", c_sz), ("g1", c_vp), ("g2", c_vp), ("inf1", c_vp), ("inf2", c_vp),
                ("s2", c_sz), ("col_g1", c_vp), ("col_inf1", c_vp), ("fixed_g2", c_vp), ("fixed_inf2", c_vp),
                ("s1", c_sz), ("col_g2", c_vp), ("col_inf2", c_vp), ("fixed_g1", c_vp), ("fixed_inf1", c_vp)]


GROTH16_POINTS_CHECKED = 1   # ZKP_GROTH16_POINTS_CHECKED
GROTH16_VK_CHECKED = 2       # ZKP_GROTH16_VK_CHECKED


class Groth16Vk(ctypes.Structure):
    """zkp_groth16_vk: a verifying key for zkp_groth16_verify_batch[_dev] (field order of include/zkp_pairings.h)"""
    _fields_ = [("alpha_g1", c_vp), ("beta_g2", c_vp), ("gamma_g2", c_vp), ("delta_g2", c_vp), ("n_inputs", c_sz), ("ic", c_vp)]


class Groth16Batch(ctypes.Structure):
    """zkp_groth16_batch: n proofs and their public inputs"""
    _fields_ = [("n", c_sz), ("a", c_vp), ("inf_a", c_vp), ("b", c_vp), ("inf_b", c_vp), ("c", c_vp), ("inf_c", c_vp), ("inputs", c_vp)]


FR_EVAL_BITREV = 1           # ZKP_FR_EVAL_BITREV
KZG_POINTS_CHECKED = 1       # ZKP_KZG_POINTS_CHECKED
KZG_VK_CHECKED = 2           # ZKP_KZG_VK_CHECKED


class KzgVk(ctypes.Structure):
    """zkp_kzg_vk: the setup points of zkp_kzg_verify_batch[_dev] (field order of include/zkp_pairings.h)"""
    _fields_ = [("g1", c_vp), ("g2", c_vp), ("tau_g2", c_vp)]


class KzgBatch(ctypes.Structure):
    """zkp_kzg_batch: n openings (commitment, proof, point, value)"""
    _fields_ = [("n", c_sz), ("c", c_vp), ("inf_c", c_vp), ("proof", c_vp), ("inf_proof", c_vp), ("z", c_vp), ("y", c_vp)]


# name -> (restype, argtypes); MUST list every symbol include/zkp_pairings.h declares
SIGNATURES = {
    "zkp_abi_version": (c_int, []),
    "zkp_strerror": (ctypes.c_char_p, [c_int]),
    "zkp_init": (c_int, [c_int, ctypes.POINTER(c_vp)]),
    "zkp_free": (None, [c_vp]),
    "zkp_last_error": (ctypes.c_char_p, [c_vp]),
    "zkp_set_validate": (c_int, [c_vp, c_int]),
    "zkp_set_kernel": (c_int, [c_vp, c_int]),
    "zkp_device_info": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.c_char_p, c_sz]),
    "zkp_gt_identity": (c_u64p, []),
    "zkp_pairing_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_multi_miller_loop_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp]),
    "zkp_final_exponentiation_batch": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "zkp_pairing_check_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, ctypes.POINTER(c_int)]),
    "zkp_miller_product": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_fp12_product": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "zkp_pairing_product_check": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(c_int)]),
    "zkp_g1_is_valid_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_g2_is_valid_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_g1_mul_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_mul_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_decode_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_decode_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_encode_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_g2_encode_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_fp_op_batch": (c_int, [c_vp, c_int, c_vp, c_vp, c_sz, c_vp]),
    "zkp_tower_op_batch": (c_int, [c_vp, c_int, c_vp, c_vp, c_sz, ctypes.c_uint32, c_vp]),
    "zkp_pairing_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_multi_miller_loop_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp]),
    "zkp_final_exponentiation_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_pairing_check_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp]),
    "zkp_pairing_gt_check_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_miller_product_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_fp12_product_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_pairing_product_check_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_is_valid_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_is_valid_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_mul_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_mul_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_decode_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_g2_decode_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_g1_encode_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_encode_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_points_check_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, ctypes.POINTER(c_int)]),
    "zkp_points_check_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "zkp_fp_sqrt_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_fp2_sqrt_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_add_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_add_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_msm_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_int, c_vp, c_vp]),
    "zkp_g2_msm_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_int, c_vp, c_vp]),
    "zkp_g1_add_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_add_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_msm_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_int, c_vp, c_vp, c_vp]),
    "zkp_g2_msm_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_int, c_vp, c_vp, c_vp]),
    "zkp_msm_profile_dev": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_sz, c_sz, c_int, c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_float)]),
    "zkp_g1_mul_endo_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_mul_endo_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_pairing_check_batch_rlc": (c_int, [c_vp, ctypes.POINTER(RlcBatch), c_vp, c_int, ctypes.POINTER(c_int)]),
    "zkp_pairing_check_batch_rlc_dev": (c_int, [c_vp, ctypes.POINTER(RlcBatch), c_vp, c_int, c_vp, c_vp]),
    "zkp_fr_op_batch": (c_int, [c_vp, c_int, c_vp, c_vp, c_sz, c_vp]),
    "zkp_fr_op_batch_dev": (c_int, [c_vp, c_int, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_fr_from_wide_batch": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "zkp_fr_from_wide_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_fr_fold_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp]),
    "zkp_fr_fold_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp]),
    "zkp_groth16_verify_batch": (c_int, [c_vp, ctypes.POINTER(Groth16Vk), ctypes.POINTER(Groth16Batch), c_vp, c_int, ctypes.POINTER(c_int)]),
    "zkp_groth16_verify_batch_dev": (c_int, [c_vp, ctypes.POINTER(Groth16Vk), ctypes.POINTER(Groth16Batch), c_vp, c_int, c_vp, c_vp]),
    "zkp_fr_invert_batch": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "zkp_fr_invert_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_fr_eval_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp]),
    "zkp_fr_eval_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp]),
    "zkp_kzg_verify_batch": (c_int, [c_vp, ctypes.POINTER(KzgVk), ctypes.POINTER(KzgBatch), c_vp, c_int, ctypes.POINTER(c_int)]),
    "zkp_kzg_verify_batch_dev": (c_int, [c_vp, ctypes.POINTER(KzgVk), ctypes.POINTER(KzgBatch), c_vp, c_int, c_vp, c_vp]),
    "zkp_g1_decompress_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_decompress_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_compress_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_g2_compress_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp]),
    "zkp_g1_decompress_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_g2_decompress_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_g1_compress_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_compress_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_points_check_compressed_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, ctypes.POINTER(c_int)]),
    "zkp_points_check_compressed_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "zkp_comm_unique_id": (c_int, [c_vp]),
    "zkp_comm_init_rank": (c_int, [c_vp, c_int, c_int, c_vp]),
    "zkp_comm_destroy": (c_int, [c_vp]),
    "zkp_comm_info": (c_int, [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "zkp_and_allreduce_dev": (c_int, [c_vp, c_vp, c_vp]),
    "zkp_pairing_check_batch_allreduce": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, ctypes.POINTER(c_int)]),
    "zkp_pairing_check_batch_allreduce_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp]),
    "zkp_pairing_gt_check_batch_allreduce_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_points_check_batch_allreduce": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, ctypes.POINTER(c_int)]),
    "zkp_points_check_batch_allreduce_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "zkp_pairing_product_check_allgather": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(c_int)]),
    "zkp_take_validation_status_dev": (c_int, [c_vp, c_vp, ctypes.POINTER(c_int)]),
    "zkp_pairing_check_batch_multi": (c_int, [ctypes.POINTER(c_vp), c_int, c_vp, c_vp, c_vp, c_vp, c_sz, c_sz, c_vp, ctypes.POINTER(c_int)]),
    "zkp_pairing_batch_multi": (c_int, [ctypes.POINTER(c_vp), c_int, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, ctypes.POINTER(c_int)]),
    "zkp_host_alloc": (c_int, [c_sz, ctypes.POINTER(c_vp)]),
    "zkp_host_free": (c_int, [c_vp]),
    "zkp_host_register": (c_int, [c_vp, c_sz]),
    "zkp_host_unregister": (c_int, [c_vp]),
    "zkp_clock_probe_dev": (c_int, [c_vp, c_vp, ctypes.c_uint, c_vp, ctypes.POINTER(c_int)]),
    "zkp_time_coop_step": (c_int, [c_vp, c_int, c_sz, ctypes.POINTER(ctypes.c_float)]),
    "zkp_profile_pairing_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(c_int)]),
    "zkp_time_pairing_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_int, ctypes.POINTER(ctypes.c_float)]),
}

NTT_INVERSE, NTT_BITREV, NTT_COSET = 1, 2, 4   # ZKP_NTT_INVERSE / _BITREV / _COSET

# name -> (restype, argtypes); MUST list every symbol include/zkp_poly.h declares (the second header of the same library)
POLY_SIGNATURES = {
    "zkp_fr_ntt_batch": (c_int, [c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp]),
    "zkp_fr_ntt_batch_dev": (c_int, [c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp]),
    "zkp_kzg_open_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp, c_vp]),
    "zkp_kzg_open_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp, c_vp, c_vp]),
}



class FrCsr(ctypes.Structure):
    """zkp_fr_csr: a sparse matrix over Fr in compressed rows (field order of include/zkp_prove.h)"""
    _fields_ = [("n_rows", c_sz), ("n_cols", c_sz), ("nnz", c_sz), ("row_ptr", c_vp), ("col", c_vp), ("val", c_vp)]


class R1cs(ctypes.Structure):
    """zkp_r1cs: the three matrices of a rank-one constraint system over the 2^log2_n-point domain"""
    _fields_ = [("log2_n", ctypes.c_uint), ("n_inputs", c_sz), ("a", FrCsr), ("b", FrCsr), ("c", FrCsr)]


class Groth16Pk(ctypes.Structure):
    """zkp_groth16_pk: a proving key for zkp_groth16_prove_batch[_dev]"""
    _fields_ = [(name, c_vp) for name in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "a_inf", "b_g1_query", "b_g1_inf",
                                          "b_g2_query", "b_g2_inf", "l_query", "l_inf", "h_query")]


# name -> (restype, argtypes); MUST list every symbol include/zkp_prove.h declares (the third header of the same library)
PROVE_SIGNATURES = {
    "zkp_fr_spmv_batch": (c_int, [c_vp, ctypes.POINTER(FrCsr), c_vp, c_sz, c_sz, c_vp]),
    "zkp_fr_spmv_batch_dev": (c_int, [c_vp, ctypes.POINTER(FrCsr), c_vp, c_sz, c_sz, c_vp, c_vp]),
    "zkp_groth16_quotient_batch": (c_int, [c_vp, ctypes.POINTER(R1cs), c_vp, c_sz, c_vp, c_vp]),
    "zkp_groth16_quotient_batch_dev": (c_int, [c_vp, ctypes.POINTER(R1cs), c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_groth16_prove_batch": (c_int, [c_vp, ctypes.POINTER(R1cs), ctypes.POINTER(Groth16Pk), c_vp, c_vp, c_sz, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "zkp_groth16_prove_batch_dev": (c_int, [c_vp, ctypes.POINTER(R1cs), ctypes.POINTER(Groth16Pk), c_vp, c_vp, c_sz, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_vp]),
}

# name -> (restype, argtypes); MUST list every symbol include/zkp_fk20.h declares (the fourth header of the same library)
FK20_SIGNATURES = {
    "zkp_g1_ntt_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp]),
    "zkp_g1_ntt_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp, c_vp]),
    "zkp_kzg_fk20_setup": (c_int, [c_vp, c_vp, ctypes.c_uint, c_vp, c_vp]),
    "zkp_kzg_fk20_setup_dev": (c_int, [c_vp, c_vp, ctypes.c_uint, c_vp, c_vp, c_vp]),
    "zkp_kzg_fk20_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp]),
    "zkp_kzg_fk20_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.c_uint, c_int, c_vp, c_vp, c_vp]),
}

# name -> (restype, argtypes); MUST list every symbol include/zkp_cells.h declares (the fifth header of the same library)
CELLS_POINTS_CHECKED, CELLS_VK_CHECKED = 4, 8   # ZKP_CELLS_POINTS_CHECKED / _VK_CHECKED
c_u = ctypes.c_uint
CELLS_SIGNATURES = {
    "zkp_kzg_cells_setup": (c_int, [c_vp, c_vp, c_u, c_u, c_vp, c_vp]),
    "zkp_kzg_cells_setup_dev": (c_int, [c_vp, c_vp, c_u, c_u, c_vp, c_vp, c_vp]),
    "zkp_kzg_cells_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_u, c_u, c_u, c_int, c_vp, c_vp]),
    "zkp_kzg_cells_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_u, c_u, c_u, c_int, c_vp, c_vp, c_vp]),
    "zkp_kzg_cell_verify_batch": (c_int, [c_vp] * 10 + [c_sz, c_u, c_u, c_int, c_vp, c_vp]),
    "zkp_kzg_cell_verify_batch_dev": (c_int, [c_vp] * 10 + [c_sz, c_u, c_u, c_int, c_vp, c_vp, c_vp]),
}

# name -> (restype, argtypes); MUST list every symbol include/zkp_recover.h declares (the sixth header of the same library)
RECOVER_SIGNATURES = {
    "zkp_das_recover_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_u, c_u, c_int, c_vp, c_vp]),
    "zkp_das_recover_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_u, c_u, c_int, c_vp, c_vp, c_vp]),
}

BLS_POINTS_CHECKED = 1       # ZKP_BLS_POINTS_CHECKED

# name -> (restype, argtypes); MUST list every symbol include/zkp_bls.h declares (hash-to-G2 and the BLS batch verifier)
BLS_SIGNATURES = {
    "zkp_fp_from_wide_be_batch": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "zkp_fp_from_wide_be_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_hash_to_field_g2_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp]),
    "zkp_hash_to_field_g2_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_map_from_fields_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_map_from_fields_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_clear_cofactor_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g2_clear_cofactor_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_hash_to_g2_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_hash_to_g2_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_bls_verify_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_verify_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp, c_vp]),
}

# name -> (restype, argtypes); MUST list every symbol include/zkp_bls_agg.h declares (G1 segment sums and FastAggregateVerify)
AGG_SIGNATURES = {
    "zkp_g1_segment_sum_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_segment_sum_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_bls_fast_aggregate_verify_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_fast_aggregate_verify_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp,
                                                        c_vp]),
}

# name -> (restype, argtypes); MUST list every symbol include/zkp_bls_grouped.h declares (scaled G1 segment sums and the verifiers grouped by message)
GRP_SIGNATURES = {
    "zkp_g1_scaled_segment_sum_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_scaled_segment_sum_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_bls_verify_grouped_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_verify_grouped_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp, c_vp]),
    "zkp_bls_fast_aggregate_verify_grouped_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int,
                                                            c_vp]),
    "zkp_bls_fast_aggregate_verify_grouped_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp,
                                                                c_int, c_vp, c_vp]),
}

# include/zkp_bls_minsig.h: hash-to-G1 and the minimal-signature-size BLS verifiers (signatures in G1, public keys in G2)
BLS_MINSIG_SIGNATURES = {
    "zkp_hash_to_field_g1_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp]),
    "zkp_hash_to_field_g1_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_map_from_fields_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_map_from_fields_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g1_clear_cofactor_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "zkp_g1_clear_cofactor_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_hash_to_g1_batch": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp]),
    "zkp_hash_to_g1_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_bls_minsig_verify_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_minsig_verify_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp, c_vp]),
    "zkp_bls_minsig_verify_samekey_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_minsig_verify_samekey_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp, c_vp]),
}

# include/zkp_bls_agg_g2.h: G2 segment sums, FastAggregateVerify for committees of G2 keys, AggregateVerify
AGG_G2_SIGNATURES = {
    "zkp_g2_segment_sum_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp]),
    "zkp_g2_segment_sum_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "zkp_bls_minsig_fast_aggregate_verify_batch": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_minsig_fast_aggregate_verify_batch_dev": (c_int, [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int,
                                                               c_vp, c_vp]),
    "zkp_bls_aggregate_verify_batch": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp]),
    "zkp_bls_aggregate_verify_batch_dev": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_int, c_vp, c_vp]),
}

_lib = None


class ZkpError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = load().zkp_strerror(status).decode()
        super().__init__("zkp status %d (%s)%s" % (status, msg, (": " + detail) if detail else ""))


def load():
    """Load the shared library (no GPU is touched by loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C zkvm_pairings_amd/csrc` (or __graft_entry__.build()). "
                "There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as the
        # system one).  Device pointers and streams are shared with torch tensors, so torch's copy must
        # be the one that is loaded first; without torch the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(POLY_SIGNATURES.items()) + list(PROVE_SIGNATURES.items()) + list(FK20_SIGNATURES.items()) +
                                  list(CELLS_SIGNATURES.items()) + list(RECOVER_SIGNATURES.items()) + list(BLS_SIGNATURES.items()) + list(AGG_SIGNATURES.items()) +
                                  list(GRP_SIGNATURES.items()) + list(BLS_MINSIG_SIGNATURES.items()) + list(AGG_G2_SIGNATURES.items())):
            fn = getattr(lib, name)  # AttributeError if the ABI lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
