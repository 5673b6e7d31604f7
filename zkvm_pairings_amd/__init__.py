"""MI355X-native batched BLS12-381 pairing engine behind the zkvm-pairings API shape.

Loading this package loads libzkp_pairings.so (the C ABI in include/zkp_pairings.h, include/zkp_poly.h, include/zkp_prove.h, include/zkp_fk20.h, include/zkp_cells.h, include/zkp_recover.h, include/zkp_bls.h, include/zkp_bls_agg.h, include/zkp_bls_grouped.h, include/zkp_bls_minsig.h and include/zkp_bls_agg_g2.h); it raises if
the library has not been built.  There is no CPU fallback."""
from . import _lib
from ._lib import ZkpError

_lib.load()

from .engine import KERNEL_AUTO, KERNEL_COOP, KERNEL_THREAD, PairingEngine  # noqa: E402
from .pairings import (R1CS, CellSetup, Fk20Setup, Fr, G1Affine, G2Affine, Groth16ProvingKey, Groth16VerifyingKey, Gt, KzgSetup, MillerLoopResult, final_exponentiation,  # noqa: E402
                       groth16_prove_batch, groth16_quotient_batch, groth16_verify_batch, groth16_verify_each, g1_ntt, kzg_commit_batch, kzg_fk20_setup, kzg_lagrange_setup, kzg_open_batch, kzg_open_domain_batch, kzg_verify_batch, kzg_verify_blob_batch, kzg_verify_each, msm,
                       kzg_cells_setup, kzg_cell_proofs_batch, kzg_cells_and_proofs_batch, kzg_cell_verify_batch, kzg_cell_verify_each,
                       recover_polynomials_batch, recover_cells_and_kzg_proofs_batch,
                       hash_to_g2, bls_sign_batch, bls_verify_batch, bls_verify_each, bls_verify_batch_compressed, bls_verify_each_compressed,
                       committee_entries, bls_aggregate_keys, bls_fast_aggregate_verify_batch, bls_fast_aggregate_verify_each,
                       group_by_message, bls_verify_grouped_batch, bls_fast_aggregate_verify_grouped_batch,
                       hash_to_g1, bls_minsig_keygen_batch, bls_minsig_sign_batch, bls_minsig_verify_batch, bls_minsig_verify_samekey_batch, bls_minsig_verify_each,
                       bls_minsig_verify_batch_compressed, bls_minsig_verify_each_compressed,
                       bls_aggregate_signatures, bls_minsig_aggregate_keys, bls_minsig_fast_aggregate_verify_batch, bls_minsig_fast_aggregate_verify_each,
                       bls_aggregate_verify_batch, bls_aggregate_verify_each,
                       multi_miller_loop, pairing)
from . import synthetic  # noqa: E402

__all__ = ["PairingEngine", "G1Affine", "G2Affine", "Gt", "MillerLoopResult", "pairing", "multi_miller_loop", "msm",
           "final_exponentiation", "Fr", "Groth16VerifyingKey", "R1CS", "Groth16ProvingKey", "groth16_prove_batch", "groth16_quotient_batch", "groth16_verify_batch", "groth16_verify_each", "KzgSetup", "kzg_verify_batch", "kzg_verify_each",
           "kzg_verify_blob_batch", "kzg_commit_batch", "kzg_open_batch", "g1_ntt", "Fk20Setup", "kzg_fk20_setup", "kzg_open_domain_batch", "kzg_lagrange_setup", "CellSetup", "kzg_cells_setup", "kzg_cell_proofs_batch", "kzg_cells_and_proofs_batch",
           "kzg_cell_verify_batch", "kzg_cell_verify_each", "recover_polynomials_batch", "recover_cells_and_kzg_proofs_batch",
           "hash_to_g2", "bls_sign_batch", "bls_verify_batch", "bls_verify_each", "bls_verify_batch_compressed", "bls_verify_each_compressed",
           "committee_entries", "bls_aggregate_keys", "bls_fast_aggregate_verify_batch", "bls_fast_aggregate_verify_each",
           "group_by_message", "bls_verify_grouped_batch", "bls_fast_aggregate_verify_grouped_batch",
           "hash_to_g1", "bls_minsig_keygen_batch", "bls_minsig_sign_batch", "bls_minsig_verify_batch", "bls_minsig_verify_samekey_batch", "bls_minsig_verify_each",
           "bls_minsig_verify_batch_compressed", "bls_minsig_verify_each_compressed",
           "bls_aggregate_signatures", "bls_minsig_aggregate_keys", "bls_minsig_fast_aggregate_verify_batch", "bls_minsig_fast_aggregate_verify_each",
           "bls_aggregate_verify_batch", "bls_aggregate_verify_each",
           "synthetic", "ZkpError", "KERNEL_AUTO", "KERNEL_THREAD", "KERNEL_COOP"]
