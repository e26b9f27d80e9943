"""ctypes binding of include/libecc_amd.h (one Python method per C entry point)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ECAMD_OK, ECAMD_ERR, ECAMD_INF = 0, 1, 2
FP_MUL_MONTY, FP_ADD, FP_SUB, FP_MUL, FP_INV = 0, 1, 2, 3, 4

# every symbol include/libecc_amd.h declares (tests check the .so exports exactly these)
EXPORTED_SYMBOLS = [
    "ecamd_device_count", "ecamd_ctx_create", "ecamd_ctx_destroy", "ecamd_last_error",
    "ecamd_ctx_set_max_chunk", "ecamd_ctx_set_secret_scalars", "ecamd_ctx_set_eddsa_msm", "ec_eddsa_verify_all_batch_dev", "ecamd_debug_eddsa_msm", "ec_eddsa_encode_point_batch", "ecamd_multi_eddsa_encode_point_batch", "ecamd_ctx_enable_kernel_timing", "ecamd_ctx_kernel_times", "ecamd_curve_by_name", "ecamd_curve_from_params", "ecamd_curve_free",
    "ecamd_curve_coord_len", "ecamd_curve_order_len", "ecamd_curve_words", "ec_prj_pt_mul_batch", "ec_prj_pt_mul_blind_batch",
    "ec_prj_pt_mul_batch_dev", "ecamd_ctx_synchronize", "ec_prj_pt_add_batch", "ec_prj_pt_dbl_batch",
    "ec_fp_op_batch", "ec_ecdsa_verify_batch", "ec_ecdsa_verify_batch_fmt", "ec_ecdsa_sign_batch", "ec_ecccdh_derive_batch", "ec_xdh_batch",
    "ec_prj_pt_mul_batch_fmt", "ec_prj_pt_unique_batch", "ec_structured_pub_key_import_batch",
    "ec_ecdsa_verify_msg_batch_fmt", "ec_eddsa_verify_msg_batch", "ecamd_multi_ecdsa_verify_msg_batch_fmt", "ecamd_multi_eddsa_verify_msg_batch",
    "ec_prj_pt_op_batch_fmt", "ec_prj_pt_unprotected_mult_batch", "ecamd_multi_prj_pt_op_batch_fmt", "ecamd_multi_prj_pt_unprotected_mult_batch",
    "ec_aff_pt_y_from_x_batch", "ec_point_decompress_batch", "ec_structured_sig_import_batch", "ec_structured_key_pair_import_batch",
    "ec_eddsa_verify_batch", "ec_eddsa_verify_all_batch", "ec_ecdsa_verify_batch_dev", "ec_eddsa_verify_batch_dev", "ec_xdh_batch_dev",
    "ec_ecdsa_sign_batch_dev", "ec_ecccdh_derive_batch_dev", "ec_eddsa_sign_R_batch", "ec_eddsa_sign_S_batch",
    "ecamd_multi_create", "ecamd_multi_destroy", "ecamd_multi_size", "ecamd_multi_device", "ecamd_multi_ctx",
    "ecamd_multi_shard_range", "ecamd_multi_curve_by_name", "ecamd_multi_curve_from_params", "ecamd_multi_curve_free",
    "ecamd_multi_curve_handle", "ecamd_multi_curve_coord_len", "ecamd_multi_curve_order_len",
    "ecamd_multi_prj_pt_mul_batch", "ecamd_multi_prj_pt_mul_batch_fmt", "ecamd_multi_prj_pt_unique_batch",
    "ecamd_multi_ecdsa_verify_batch", "ecamd_multi_ecdsa_verify_batch_fmt", "ecamd_multi_ecdsa_sign_batch", "ecamd_multi_ecccdh_derive_batch",
    "ecamd_multi_xdh_batch", "ecamd_multi_eddsa_verify_batch", "ecamd_multi_eddsa_verify_all_batch", "ecamd_multi_allgather",
    "ecamd_multi_allgather_streams", "ecamd_multi_eddsa_sign_R_batch", "ecamd_multi_eddsa_sign_S_batch",
    "ecamd_multi_set_secret_scalars", "ecamd_multi_wipe_scratch", "ecamd_ctx_wipe_scratch", "ecamd_ctx_stream", "ecamd_host_alloc", "ecamd_host_free", "ecamd_ctx_dominant_kernel_ms", "ecamd_ctx_set_msm_seed", "ecamd_ctx_discard_msm_seed", "ecamd_multi_set_msm_seed", "ec_eddsa_verify_ph_prj_batch", "ecamd_multi_eddsa_verify_ph_prj_batch", "ec_nn_random_mod_batch", "ec_ecdsa_sign_msg_batch", "ec_key_pair_gen_raw_batch", "ecamd_multi_ecdsa_sign_msg_batch", "ecamd_multi_key_pair_gen_raw_batch", "ec_eddsa_verify_msg_prj_batch", "ecamd_multi_eddsa_verify_msg_prj_batch", "ecamd_ctx_set_host_ready_hook", "ecamd_multi_set_host_ready_hook", "ecamd_multi_prj_pt_add_batch",
    "ec_schnorr_verify_all_batch", "ec_schnorr_verify_all_batch_dev", "ec_schnorr_verify_msg_all_batch", "ec_eddsa_verify_msg_prj_all_batch", "ecamd_multi_eddsa_verify_msg_prj_all_batch", "ecamd_multi_schnorr_verify_msg_all_batch", "ec_schnorr_verify_all_available", "ecamd_multi_schnorr_verify_all_batch", "ecamd_debug_schnorr_msm", "ecamd_debug_schnorr_msm_words",
    "ec_ecdsa_recover_batch", "ec_ecdsa_recover_batch_dev",
    "ec_sig_verify_batch", "ec_sig_verify_batch_dev", "ec_sig_sign_batch", "ec_sig_sign_batch_dev",
    "ec_sig_verify_msg_batch", "ec_sig_verify_msg_batch_dev", "ec_sig_sign_msg_batch", "ec_sig_sign_msg_batch_dev",
    "ec_hash_slots_batch", "ec_hash_slots_batch_dev",
    "ecamd_digest_len", "ec_digest_slots_batch", "ec_digest_slots_batch_dev",
    "ec_sig_hashed_verify_batch", "ec_sig_hashed_verify_batch_dev", "ec_sig_hashed_sign_batch", "ec_sig_hashed_sign_batch_dev",
    "ec_schnorr_verify_batch", "ec_schnorr_verify_batch_dev", "ec_schnorr_sign_batch", "ec_schnorr_sign_batch_dev",
    "ec_bign_verify_batch", "ec_bign_verify_batch_dev", "ec_bign_sign_batch", "ec_bign_sign_batch_dev",
    "ec_rfc6979_nonce_batch", "ec_rfc6979_nonce_batch_dev", "ec_decdsa_sign_batch", "ec_decdsa_sign_batch_dev",
    "ec_hmac_slots_batch", "ec_hmac_slots_batch_dev", "ec_rfc6979_nonce_ht_batch", "ec_rfc6979_nonce_ht_batch_dev",
    "ec_decdsa_sign_ht_batch", "ec_decdsa_sign_ht_batch_dev",
    "ec_eddsa_sign_msg_batch", "ec_eddsa_sign_msg_batch_dev", "ec_eddsa_pub_key_batch", "ec_eddsa_pub_key_batch_dev",
    "ec_dbign_nonce_batch", "ec_dbign_nonce_batch_dev", "ec_dbign_sign_batch", "ec_dbign_sign_batch_dev",
    "ec_bip0340_nonce_batch", "ec_bip0340_nonce_batch_dev", "ec_bip0340_sign_batch", "ec_bip0340_sign_batch_dev",
    "ec_sig_hashed_verify_ht_batch", "ec_sig_hashed_verify_ht_batch_dev", "ec_sig_hashed_sign_ht_batch", "ec_sig_hashed_sign_ht_batch_dev",
    "ec_schnorr_verify_ht_batch", "ec_schnorr_verify_ht_batch_dev", "ec_schnorr_sign_ht_batch", "ec_schnorr_sign_ht_batch_dev",
    "ec_bip0340_nonce_ht_batch", "ec_bip0340_nonce_ht_batch_dev", "ec_bip0340_sign_ht_batch", "ec_bip0340_sign_ht_batch_dev",
    "ec_digest_msgs_batch", "ec_digest_msgs_batch_dev", "ec_ecdsa_verify_msgs_batch", "ec_ecdsa_verify_msgs_batch_dev",
    "ec_decdsa_sign_msgs_batch", "ec_decdsa_sign_msgs_batch_dev",
    "ec_eddsa_verify_msgs_batch", "ec_eddsa_verify_msgs_batch_dev", "ec_eddsa_verify_msgs_all_batch", "ec_eddsa_verify_msgs_all_batch_dev",
    "ec_eddsa_sign_msgs_batch", "ec_eddsa_sign_msgs_batch_dev",
]

# libecc's ec_alg_type numbers of the EdDSA variants ec_eddsa_sign_msg_batch serves (lib_ecc_types.h:49-55)
EDDSA25519, EDDSA25519CTX, EDDSA25519PH, EDDSA448, EDDSA448PH = 9, 10, 11, 12, 13

# libecc's ec_alg_type numbers of the schemes ec_sig_verify_batch / ec_sig_sign_batch serve (ECAMD_SIG_* in include/libecc_amd.h)
SIG_ECGDSA, SIG_ECRDSA, SIG_SM2 = 6, 7, 8
# ... and of the schemes that hash the commitment, served by ec_sig_hashed_verify_batch / ec_sig_hashed_sign_batch
SIG_ECKCDSA, SIG_ECSDSA, SIG_ECOSDSA = 2, 3, 4
# ... and of the two Schnorr-type schemes with a point commitment, served item by item by ec_schnorr_verify_batch / ec_schnorr_sign_batch
SIG_ECFSDSA, SIG_BIP0340 = 5, 20
# ... and of BIGN / DBIGN (STB 34.101.45), served by ec_bign_verify_batch / ec_bign_sign_batch; HASH_BELT: libecc's hash_alg_type
# number of belt-hash, which those calls (and only those) compute on the device beside SHA-2
SIG_BIGN, SIG_DBIGN = 18, 19
HASH_BELT = 16
HASH_SIZES = {1: 28, 2: 32, 3: 48, 4: 64}          # libecc's hash_alg_type numbers of SHA-224 / 256 / 384 / 512
HASH_SM3, HASH_STREEBOG256, HASH_STREEBOG512 = 11, 13, 14
HASH_SLOT_SIZES = {**HASH_SIZES, 11: 32, 13: 32, 14: 64}   # what ec_hash_slots_batch and the message-level ec_sig_* calls hash with
# what ec_digest_slots_batch hashes with: every fixed-length hash of libecc's table but belt-hash -- beside the seven above SHA3-224 /
# 256 / 384 / 512 (5 .. 8), SHA-512/224 and /256 (9, 10), RIPEMD-160 (15) and BASH224 / 256 / 384 / 512 (17 .. 20)
DIGEST_SIZES = {**HASH_SLOT_SIZES, 5: 28, 6: 32, 7: 48, 8: 64, 9: 28, 10: 32, 15: 20, 17: 28, 18: 32, 19: 48, 20: 64}


class EcamdError(RuntimeError):
    pass


def pack_msgs(msgs):
    """a list of `bytes` as the packed array and the n + 1 u64 offsets of the ec_*_msgs_batch calls"""
    offs, pos = (C.c_uint64 * (len(msgs) + 1))(), 0
    for i, m in enumerate(msgs):
        pos += len(m)
        offs[i + 1] = pos
    return b"".join(msgs), offs


def lib_path():
    # ECAMD_LIB_PATH: developer override to A/B-test an alternative build of the same library
    return os.environ.get("ECAMD_LIB_PATH") or os.path.join(HERE, "lib", "libecc_amd.so")


_LIB = None


def load_library():
    """Load the HIP shared library; raises (never falls back) if it has not been built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise EcamdError(f"{path} is missing: run `python libecc_amd/build.py` "
                             "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(path)
        vp, u8p, u32 = C.c_void_p, C.c_char_p, C.c_uint32
        L.ecamd_last_error.restype = C.c_char_p
        L.ecamd_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
        L.ecamd_ctx_destroy.argtypes = [vp]
        L.ecamd_ctx_destroy.restype = None
        L.ecamd_ctx_set_max_chunk.argtypes = [vp, u32]
        L.ecamd_ctx_set_secret_scalars.argtypes = [vp, C.c_int]
        L.ecamd_ctx_synchronize.argtypes = [vp]
        L.ecamd_ctx_enable_kernel_timing.argtypes = [vp, C.c_int]
        L.ecamd_ctx_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
        L.ecamd_curve_by_name.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.ecamd_curve_from_params.argtypes = [vp] + [u8p, u32] * 7 + [C.POINTER(vp)]
        L.ecamd_curve_free.argtypes = [vp]
        L.ecamd_curve_free.restype = None
        for f in ("ecamd_curve_coord_len", "ecamd_curve_order_len", "ecamd_curve_words"):
            getattr(L, f).argtypes = [vp]
        L.ec_prj_pt_mul_batch.argtypes = [vp, vp, u32, u8p, u32, u8p, u8p, u8p]
        L.ec_prj_pt_mul_blind_batch.argtypes = [vp, vp, u32, u8p, u32, u8p, u32, u8p, u8p, u8p]
        L.ec_prj_pt_mul_batch_dev.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, vp]
        L.ec_prj_pt_add_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ec_prj_pt_dbl_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ec_fp_op_batch.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp]
        L.ec_ecdsa_verify_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p]
        L.ec_ecdsa_sign_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_ecdsa_verify_batch_fmt.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, u8p, u32, u8p]
        L.ec_xdh_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ec_eddsa_verify_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p]
        L.ec_eddsa_verify_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
        L.ecamd_debug_eddsa_msm.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p, C.POINTER(C.c_int), vp, vp]
        L.ecamd_ctx_set_eddsa_msm.argtypes = [vp, C.c_int, u32, u32]
        L.ec_schnorr_verify_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p, C.c_int, C.POINTER(C.c_int)]
        L.ec_schnorr_verify_all_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, C.c_int, vp, vp]
        L.ec_eddsa_verify_msg_prj_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u32, C.POINTER(C.c_int)]
        L.ecamd_multi_eddsa_verify_msg_prj_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u32, C.POINTER(C.c_int)]
        L.ec_schnorr_verify_msg_all_batch.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, C.c_int, C.c_int, u8p, u32, u32, C.POINTER(C.c_int)]
        L.ecamd_multi_schnorr_verify_msg_all_batch.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, C.c_int, C.c_int, u8p, u32, u32, C.POINTER(C.c_int)]
        L.ecamd_multi_schnorr_verify_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p, C.c_int, C.POINTER(C.c_int)]
        L.ec_schnorr_verify_all_available.argtypes = [vp, C.c_int]
        L.ecamd_debug_schnorr_msm.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p, C.c_int, u8p, C.POINTER(C.c_int), vp, vp]
        L.ecamd_debug_schnorr_msm_words.argtypes = [vp]
        L.ecamd_debug_schnorr_msm_words.restype = C.c_uint32
        L.ec_eddsa_verify_all_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp]
        L.ec_eddsa_encode_point_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ecamd_multi_eddsa_encode_point_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ec_prj_pt_mul_batch_fmt.argtypes = [vp, vp, u32, u8p, u32, u8p, C.c_int, u8p, C.c_int, u8p]
        L.ec_prj_pt_unique_batch.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, C.c_int, u8p]
        L.ec_structured_pub_key_import_batch.argtypes = [vp, vp, u32, u8p, u32, C.c_int, u8p, u8p]
        L.ec_aff_pt_y_from_x_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ec_point_decompress_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ec_structured_sig_import_batch.argtypes = [vp, u32, u8p, u32, C.c_int, C.c_int, u8p, u8p]
        L.ec_structured_key_pair_import_batch.argtypes = [vp, vp, u32, u8p, u32, C.c_int, u8p, u8p, u8p]
        L.ec_ecdsa_verify_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp]
        L.ec_sig_verify_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p]
        L.ec_sig_sign_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_sig_verify_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, u32, vp, vp]
        L.ec_sig_sign_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, u32, vp, vp, vp]
        L.ec_sig_verify_msg_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u32, u8p]
        L.ec_sig_verify_msg_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, u32, u8p, u32, vp, vp]
        L.ec_sig_sign_msg_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u8p, u32, u8p, u32, u8p, u8p]
        L.ec_sig_sign_msg_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, vp, u32, u8p, u32, vp, vp, vp]
        L.ec_hash_slots_batch.argtypes = [vp, C.c_int, u32, u8p, u32, u8p]
        L.ec_hash_slots_batch_dev.argtypes = [vp, C.c_int, u32, vp, u32, vp, vp]
        L.ecamd_digest_len.argtypes = [C.c_int]
        L.ec_digest_slots_batch.argtypes = [vp, C.c_int, u32, u8p, u32, u8p]
        L.ec_digest_slots_batch_dev.argtypes = [vp, C.c_int, u32, vp, u32, vp, vp]
        u64 = C.c_uint64
        L.ec_digest_msgs_batch.argtypes = [vp, C.c_int, u32, u8p, vp, u8p, u32, u8p, u32, u32, u8p, u8p]
        L.ec_digest_msgs_batch_dev.argtypes = [vp, C.c_int, u32, vp, u64, vp, u8p, u32, vp, u32, u32, vp, vp, vp]
        L.ec_ecdsa_verify_msgs_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, vp, u8p]
        L.ec_ecdsa_verify_msgs_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, u64, vp, vp, vp]
        L.ec_decdsa_sign_msgs_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, vp, u8p, u8p]
        L.ec_decdsa_sign_msgs_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u64, vp, vp, vp, vp]
        L.ec_sig_hashed_verify_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u32, u8p]
        L.ec_sig_hashed_sign_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_sig_hashed_verify_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, u32, vp, vp]
        L.ec_sig_hashed_sign_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, u32, vp, vp, vp]
        L.ec_bign_verify_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u32, u8p]
        L.ec_bign_sign_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u32, u8p, u8p]
        L.ec_bign_verify_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, u32, u8p, u32, vp, vp]
        L.ec_bign_sign_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, u32, u8p, u32, vp, vp, vp]
        L.ec_schnorr_verify_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, C.c_int, u8p, u8p, u32, u8p]
        L.ec_schnorr_sign_batch.argtypes = [vp, vp, C.c_int, C.c_int, u32, u8p, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_schnorr_verify_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, C.c_int, vp, vp, u32, vp, vp]
        L.ec_schnorr_sign_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, u32, vp, vp, vp, vp, u32, vp, vp, vp]
        L.ec_ecdsa_recover_batch.argtypes = [vp, vp, u32, u8p, u8p, u32, u8p, u8p, u8p, u8p]
        L.ec_ecdsa_recover_batch_dev.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp]
        L.ec_eddsa_verify_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp]
        L.ec_eddsa_sign_R_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ec_eddsa_sign_S_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ec_ecdsa_sign_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]
        L.ec_rfc6979_nonce_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u8p]
        L.ec_rfc6979_nonce_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, vp, vp]
        L.ec_decdsa_sign_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u32, C.c_int, u8p, u8p]
        L.ec_decdsa_sign_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u32, C.c_int, vp, vp, vp]
        L.ec_hmac_slots_batch.argtypes = [vp, C.c_int, u32, u8p, u32, u8p, u32, u8p]
        L.ec_hmac_slots_batch_dev.argtypes = [vp, C.c_int, u32, vp, u32, vp, u32, vp, vp]
        L.ec_rfc6979_nonce_ht_batch.argtypes = L.ec_rfc6979_nonce_batch.argtypes
        L.ec_rfc6979_nonce_ht_batch_dev.argtypes = L.ec_rfc6979_nonce_batch_dev.argtypes
        L.ec_decdsa_sign_ht_batch.argtypes = L.ec_decdsa_sign_batch.argtypes
        L.ec_decdsa_sign_ht_batch_dev.argtypes = L.ec_decdsa_sign_batch_dev.argtypes
        L.ec_dbign_nonce_batch.argtypes = [vp, vp, u32, u8p, u8p, u32, u8p, u32, u8p, u32, u8p, u8p]
        L.ec_dbign_nonce_batch_dev.argtypes = [vp, vp, u32, vp, vp, u32, u8p, u32, u8p, u32, vp, vp, vp]
        L.ec_dbign_sign_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u32, u8p, u32, u8p, u32, u8p, u8p]
        L.ec_dbign_sign_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u32, u8p, u32, u8p, u32, vp, vp, vp]
        L.ec_bip0340_nonce_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_bip0340_nonce_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, vp, u32, vp, vp, vp]
        L.ec_bip0340_sign_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u8p, u32, u8p, u8p]
        L.ec_bip0340_sign_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, vp, vp, u32, vp, vp, vp]
        # the _ht forms: the same arguments, hash_type from DIGEST_SIZES
        for base in ("ec_sig_hashed_verify", "ec_sig_hashed_sign", "ec_schnorr_verify", "ec_schnorr_sign", "ec_bip0340_nonce", "ec_bip0340_sign"):
            for tail in ("_batch", "_batch_dev"):
                getattr(L, base + "_ht" + tail).argtypes = getattr(L, base + tail).argtypes
        L.ec_eddsa_sign_msg_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p, u32, u8p, u8p, u8p]
        L.ec_eddsa_sign_msg_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u8p, u32, vp, u32, vp, vp, vp, vp]
        L.ec_eddsa_verify_msgs_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p, vp, u8p]
        L.ec_eddsa_verify_msgs_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u8p, u32, vp, u64, vp, vp, vp]
        L.ec_eddsa_verify_msgs_all_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
        L.ec_eddsa_verify_msgs_all_batch_dev.argtypes = L.ec_eddsa_verify_msgs_batch_dev.argtypes
        L.ec_eddsa_sign_msgs_batch.argtypes = [vp, vp, C.c_int, u32, u8p, u8p, u8p, u32, u8p, vp, u8p, u8p, u8p]
        L.ec_eddsa_sign_msgs_batch_dev.argtypes = [vp, vp, C.c_int, u32, vp, vp, u8p, u32, vp, u64, vp, vp, vp, vp, vp]
        L.ec_eddsa_pub_key_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p]
        L.ec_eddsa_pub_key_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
        L.ec_ecccdh_derive_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
        L.ec_xdh_batch_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
        L.ec_ecccdh_derive_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        # several GPUs from C
        L.ecamd_multi_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
        L.ecamd_multi_destroy.argtypes = [vp]
        L.ecamd_multi_destroy.restype = None
        L.ecamd_multi_size.argtypes = [vp]
        L.ecamd_multi_device.argtypes = [vp, C.c_int]
        L.ecamd_multi_ctx.argtypes = [vp, C.c_int]
        L.ecamd_multi_ctx.restype = vp
        L.ecamd_multi_shard_range.argtypes = [u32, C.c_int, C.c_int, C.POINTER(u32), C.POINTER(u32)]
        L.ecamd_multi_shard_range.restype = None
        L.ecamd_multi_curve_by_name.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
        L.ecamd_multi_curve_from_params.argtypes = [vp] + [u8p, u32] * 7 + [C.POINTER(vp)]
        L.ecamd_multi_curve_free.argtypes = [vp]
        L.ecamd_multi_curve_free.restype = None
        L.ecamd_multi_curve_handle.argtypes = [vp, C.c_int]
        L.ecamd_multi_curve_handle.restype = vp
        L.ecamd_multi_curve_coord_len.argtypes = [vp]
        L.ecamd_multi_curve_order_len.argtypes = [vp]
        L.ecamd_multi_prj_pt_mul_batch.argtypes = [vp, vp, u32, u8p, u32, u8p, u8p, u8p]
        L.ecamd_multi_prj_pt_mul_batch_fmt.argtypes = [vp, vp, u32, u8p, u32, u8p, C.c_int, u8p, C.c_int, u8p]
        L.ecamd_multi_prj_pt_unique_batch.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, C.c_int, u8p]
        L.ecamd_multi_ecdsa_verify_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p]
        L.ecamd_multi_ecdsa_verify_batch_fmt.argtypes = [vp, vp, u32, u8p, C.c_int, u8p, u8p, u32, u8p]
        L.ecamd_multi_ecdsa_sign_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p, u8p]
        L.ecamd_multi_ecccdh_derive_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ecamd_multi_xdh_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u8p]
        L.ecamd_multi_eddsa_verify_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, u8p]
        L.ecamd_multi_eddsa_verify_all_batch.argtypes = [vp, vp, u32, u8p, u8p, u8p, u32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
        L.ecamd_multi_allgather.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_size_t]
        _LIB = L
    return _LIB


def _chk(L, ret, what):
    if ret != 0:
        raise EcamdError(f"{what}: {L.ecamd_last_error().decode()}")


class Context:
    """ecamd_ctx: one GPU."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        _chk(self.L, self.L.ecamd_ctx_create(C.byref(self.h), device), "ecamd_ctx_create")

    def close(self):
        if self.h:
            self.L.ecamd_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def set_max_chunk(self, n):
        _chk(self.L, self.L.ecamd_ctx_set_max_chunk(self.h, n), "ecamd_ctx_set_max_chunk")

    def hash_slots(self, hash_type, slots, stride):
        """the bare device hash of message slots (1 .. 4 SHA-2, 11 SM3, 13 / 14 Streebog-256 / -512): n x digest size bytes"""
        n = len(slots) // stride
        hl = HASH_SLOT_SIZES.get(hash_type, 0)
        out = C.create_string_buffer(max(1, n * hl))
        _chk(self.L, self.L.ec_hash_slots_batch(self.h, hash_type, n, slots, stride, out), "ec_hash_slots_batch")
        return out.raw[:n * hl]

    def hash_slots_dev(self, hash_type, n, d_slots, stride, d_digests, stream=None):
        _chk(self.L, self.L.ec_hash_slots_batch_dev(self.h, hash_type, n, d_slots, stride, d_digests, stream), "ec_hash_slots_batch_dev")

    def digest_slots(self, hash_type, slots, stride):
        """the bare device hash of message slots over the whole table (DIGEST_SIZES): n x digest size bytes; a slot that does not fit
        its stride gives zeros"""
        n = len(slots) // stride
        dl = DIGEST_SIZES.get(hash_type, 0)
        out = C.create_string_buffer(max(1, n * dl))
        _chk(self.L, self.L.ec_digest_slots_batch(self.h, hash_type, n, slots, stride, out), "ec_digest_slots_batch")
        return out.raw[:n * dl]

    def digest_slots_dev(self, hash_type, n, d_slots, stride, d_digests, stream=None):
        _chk(self.L, self.L.ec_digest_slots_batch_dev(self.h, hash_type, n, d_slots, stride, d_digests, stream), "ec_digest_slots_batch_dev")

    def digest_msgs(self, hash_type, msgs, call_prefix=b"", item_prefixes=None):
        """the device hash over the whole table (DIGEST_SIZES) of call_prefix || item_prefixes[i] || msgs[i] for a list of `bytes` of any
        lengths, through the packed array and its offsets: (n x digest size bytes, n status bytes -- 1 with a zero digest where the
        input exceeds 2^28 octets).  item_prefixes: a list of n `bytes` of one length (at most 256), or None"""
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        ipl = len(item_prefixes[0]) if item_prefixes else 0
        assert item_prefixes is None or (len(item_prefixes) == n and all(len(p) == ipl for p in item_prefixes))
        dl = DIGEST_SIZES.get(hash_type, 0)
        out, st = C.create_string_buffer(max(1, n * dl)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_digest_msgs_batch(self.h, hash_type, n, packed, offs, call_prefix, len(call_prefix),
                                                 b"".join(item_prefixes) if ipl else None, ipl, ipl, out, st), "ec_digest_msgs_batch")
        return out.raw[:n * dl], st.raw[:n]

    def digest_msgs_dev(self, hash_type, n, d_msgs, msgs_len, d_offsets, d_digests, d_status=None, call_prefix=b"", d_item_prefixes=None,
                        item_prefix_len=0, item_prefix_stride=0, stream=None):
        """the same on device pointers (d_msgs 4-byte aligned and readable up to round_up(msgs_len, 4); d_offsets n + 1 u64); only enqueues"""
        _chk(self.L, self.L.ec_digest_msgs_batch_dev(self.h, hash_type, n, d_msgs, msgs_len, d_offsets, call_prefix, len(call_prefix), d_item_prefixes,
                                                     item_prefix_len, item_prefix_stride, d_digests, d_status, stream), "ec_digest_msgs_batch_dev")

    def hmac_slots(self, hash_type, key_slots, key_stride, msg_slots, stride):
        """HMAC over any hash of DIGEST_SIZES of n (key slot, message slot) pairs: n x digest size bytes; a key or a message that does
        not fit its slot gives zeros"""
        n = len(msg_slots) // stride
        dl = DIGEST_SIZES.get(hash_type, 0)
        out = C.create_string_buffer(max(1, n * dl))
        _chk(self.L, self.L.ec_hmac_slots_batch(self.h, hash_type, n, key_slots, key_stride, msg_slots, stride, out), "ec_hmac_slots_batch")
        return out.raw[:n * dl]

    def hmac_slots_dev(self, hash_type, n, d_key_slots, key_stride, d_msg_slots, stride, d_macs, stream=None):
        _chk(self.L, self.L.ec_hmac_slots_batch_dev(self.h, hash_type, n, d_key_slots, key_stride, d_msg_slots, stride, d_macs, stream),
             "ec_hmac_slots_batch_dev")

    def set_secret_scalars(self, on=True):
        _chk(self.L, self.L.ecamd_ctx_set_secret_scalars(self.h, 1 if on else 0), "ecamd_ctx_set_secret_scalars")

    def set_eddsa_msm(self, mode=1, min_items=0, items_per_lane=0):
        """Ed25519 whole-batch verification through the multi-scalar multiplication: 0 never, 1 large batches, 2 always"""
        _chk(self.L, self.L.ecamd_ctx_set_eddsa_msm(self.h, mode, min_items, items_per_lane), "ecamd_ctx_set_eddsa_msm")

    def set_host_ready_hook(self, fn):
        """ecamd_ctx_set_host_ready_hook: fn(first, count) is called before the host-pointer entry points read that range of their
        input arrays (None clears it)"""
        HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32)
        self._hook = HOOK((lambda arg, first, count: fn(first, count))) if fn else C.cast(None, HOOK)   # kept alive with the context
        self.L.ecamd_ctx_set_host_ready_hook.argtypes = [C.c_void_p, HOOK, C.c_void_p]
        self.L.ecamd_ctx_set_host_ready_hook.restype = C.c_int
        _chk(self.L, self.L.ecamd_ctx_set_host_ready_hook(self.h, self._hook, None), "ecamd_ctx_set_host_ready_hook")

    def enable_kernel_timing(self, on=True):
        _chk(self.L, self.L.ecamd_ctx_enable_kernel_timing(self.h, 1 if on else 0), "ecamd_ctx_enable_kernel_timing")

    def kernel_times(self):
        """ms of [table, affine, loop, finalize] of the last fast-path batch (HIP events on its stream)"""
        ms = (C.c_double * 4)()
        _chk(self.L, self.L.ecamd_ctx_kernel_times(self.h, ms, 4), "ecamd_ctx_kernel_times")
        return list(ms)

    def dominant_kernel_ms(self):
        """ms of the dominant kernel of the last protocol call (verify loop / ladder / Edwards window loop), timing enabled"""
        ms = C.c_double(0.0)
        _chk(self.L, self.L.ecamd_ctx_dominant_kernel_ms(self.h, C.byref(ms)), "ecamd_ctx_dominant_kernel_ms")
        return ms.value

    def synchronize(self):
        _chk(self.L, self.L.ecamd_ctx_synchronize(self.h), "ecamd_ctx_synchronize")

    def curve(self, name):
        return Curve(self, name)


class Curve:
    """ecamd_curve: the ec_params equivalent, bound to a context."""

    def __init__(self, ctx, name=None, params=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        if params is None:
            _chk(self.L, self.L.ecamd_curve_by_name(ctx.h, name.encode(), C.byref(self.h)),
                 "ecamd_curve_by_name")
        else:
            args = []
            for k in ("p", "a", "b", "order", "gx", "gy", "q"):
                v = params[k]
                b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
                args += [b, len(b)]
            _chk(self.L, self.L.ecamd_curve_from_params(ctx.h, *args, C.byref(self.h)),
                 "ecamd_curve_from_params")
        self.name = name
        self.clen = self.L.ecamd_curve_coord_len(self.h)
        self.qlen = self.L.ecamd_curve_order_len(self.h)
        self.words = self.L.ecamd_curve_words(self.h)

    def free(self):
        if self.h:
            self.L.ecamd_curve_free(self.h)
            self.h = C.c_void_p()

    # -- batched prj_pt_mul, host buffers (bytes in, bytes out) --
    def scalar_mult(self, scalars, points=None, slen=None):
        slen = slen or self.qlen
        n = len(scalars) // slen
        out = C.create_string_buffer(max(1, 2 * self.clen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_mul_batch(self.ctx.h, self.h, n, scalars, slen, points, out, st),
             "ec_prj_pt_mul_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]

    def scalar_mult_blind(self, scalars, blinds, points=None, slen=None, blen=None):
        """prj_pt_mul_blind: the device multiplies by m + b #E"""
        slen, blen = slen or self.qlen, blen or self.qlen
        n = len(scalars) // slen
        out, st = C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_mul_blind_batch(self.ctx.h, self.h, n, scalars, slen, blinds, blen, points, out, st),
             "ec_prj_pt_mul_blind_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]

    # -- batched prj_pt_mul, device pointers (e.g. torch tensors' data_ptr()), asynchronous --
    def scalar_mult_dev(self, n, d_scalars, slen, d_points, d_out, d_status, stream=None):
        _chk(self.L, self.L.ec_prj_pt_mul_batch_dev(self.ctx.h, self.h, n, d_scalars, slen, d_points,
                                                     d_out, d_status, stream),
             "ec_prj_pt_mul_batch_dev")

    def pt_add(self, p1, p2=None):
        n = len(p1) // (2 * self.clen)
        out = C.create_string_buffer(max(1, 2 * self.clen * n))
        st = C.create_string_buffer(max(1, n))
        if p2 is None:
            _chk(self.L, self.L.ec_prj_pt_dbl_batch(self.ctx.h, self.h, n, p1, out, st), "ec_prj_pt_dbl_batch")
        else:
            _chk(self.L, self.L.ec_prj_pt_add_batch(self.ctx.h, self.h, n, p1, p2, out, st),
                 "ec_prj_pt_add_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]

    def fp_op(self, op, a, b):
        """a, b: lists of Python ints < p; returns a list of ints (libecc 64-bit limb layout inside)."""
        n = len(a)
        nl = (self.clen * 8 + 63) // 64
        mask = 2**64 - 1
        A = (C.c_uint64 * (n * nl))(*[(x >> (64 * k)) & mask for x in a for k in range(nl)])
        B = (C.c_uint64 * (n * nl))(*[(x >> (64 * k)) & mask for x in b for k in range(nl)])
        O = (C.c_uint64 * (n * nl))()
        _chk(self.L, self.L.ec_fp_op_batch(self.ctx.h, self.h, op, n, A, B, O), "ec_fp_op_batch")
        return [sum(O[i * nl + k] << (64 * k) for k in range(nl)) for i in range(n)]

    # -- protocol callers --
    def ecdsa_verify(self, pubs, sigs, digests, hlen):
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_verify_batch(self.ctx.h, self.h, n, pubs, sigs, digests, hlen, res),
             "ec_ecdsa_verify_batch")
        return res.raw[:n]

    def ecdsa_recover(self, sigs, digests, hlen):
        """ecdsa_public_key_from_sig: (pub1, pub2, status1, status2), the reference's two candidate keys (affine X || Y) per
        (signature, digest) pair; ECAMD_ERR in both statuses where the reference returns -1, ECAMD_INF for a key at infinity"""
        n = len(sigs) // (2 * self.qlen)
        p1, p2 = C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, 2 * self.clen * n))
        s1, s2 = C.create_string_buffer(max(1, n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_recover_batch(self.ctx.h, self.h, n, sigs, digests, hlen, p1, p2, s1, s2),
             "ec_ecdsa_recover_batch")
        return p1.raw[:2 * self.clen * n], p2.raw[:2 * self.clen * n], s1.raw[:n], s2.raw[:n]

    @staticmethod
    def msg_slots(msgs, stride=None):
        """fixed-stride slots (u32 little-endian length + bytes) of a list of messages, as the *_msg_* entry points take them"""
        stride = stride or ((4 + max([len(m) for m in msgs] + [0]) + 3) // 4) * 4
        buf = bytearray(stride * len(msgs))
        for i, m in enumerate(msgs):
            buf[stride * i:stride * i + 4] = len(m).to_bytes(4, "little")
            buf[stride * i + 4:stride * i + 4 + len(m)] = m
        return bytes(buf), stride

    def ecdsa_verify_msgs(self, pubs, pub_fmt, sigs, hash_type, msgs):
        """ECDSA verification with H(m) computed on the device (hash_type 1..4 = SHA-224/256/384/512); msgs: list of bytes"""
        n = len(msgs)
        slots, stride = self.msg_slots(msgs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_verify_msg_batch_fmt(self.ctx.h, self.h, n, pubs, pub_fmt, sigs, hash_type, slots, stride, res),
             "ec_ecdsa_verify_msg_batch_fmt")
        return res.raw[:n]

    def eddsa_verify_msgs(self, pubkeys, sigs, hash_inputs):
        """Ed25519 verification with hram = SHA-512(dom2 || R || A || PH(M)) computed on the device; hash_inputs: list of bytes"""
        n = len(hash_inputs)
        slots, stride = self.msg_slots(hash_inputs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_verify_msg_batch(self.ctx.h, self.h, n, pubkeys, sigs, slots, stride, res), "ec_eddsa_verify_msg_batch")
        return res.raw[:n]

    def eddsa_verify_msgs_prj(self, keys_prj, sigs, hash_inputs, a_offset):
        """the same from projective keys (X || Y || Z on WEI25519): the device writes each key's encoding into bytes
        a_offset .. a_offset + 32 of its hash input (left blank by the caller) before hashing"""
        n = len(hash_inputs)
        slots, stride = self.msg_slots(hash_inputs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_verify_msg_prj_batch(self.ctx.h, self.h, n, keys_prj, sigs, slots, stride, a_offset, res),
             "ec_eddsa_verify_msg_prj_batch")
        return res.raw[:n]

    def eddsa_verify_ph_prj(self, keys_prj, sigs, hash_inputs, a_offset, msgs):
        """EDDSA25519PH from projective keys: hash_inputs hold dom2 || R || 96 blank octets (A, PH(M)) at a_offset; the device hashes
        msgs, fills both blanks, hashes again and verifies"""
        n = len(hash_inputs)
        slots, stride = self.msg_slots(hash_inputs)
        mslots, mstride = self.msg_slots(msgs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_verify_ph_prj_batch(self.ctx.h, self.h, n, keys_prj, sigs, slots, stride, a_offset, mslots, mstride, res),
             "ec_eddsa_verify_ph_prj_batch")
        return res.raw[:n]

    def ecdsa_verify_fmt(self, pubs, pub_fmt, sigs, digests, hlen):
        n = len(pubs) // ((3 if pub_fmt else 2) * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_verify_batch_fmt(self.ctx.h, self.h, n, pubs, pub_fmt, sigs, digests, hlen, res),
             "ec_ecdsa_verify_batch_fmt")
        return res.raw[:n]

    def ecdsa_sign(self, privs, nonces, digests, hlen):
        n = len(privs) // self.qlen
        sigs = C.create_string_buffer(max(1, 2 * self.qlen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_sign_batch(self.ctx.h, self.h, n, privs, nonces, digests, hlen, sigs, st),
             "ec_ecdsa_sign_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def sig_verify(self, alg, pubs, sigs, digests, hlen):
        """ECGDSA / ECRDSA / SM2 verification (alg: SIG_ECGDSA, SIG_ECRDSA, SIG_SM2): 0 accept / 1 reject per item.  digests are the
        bytes the scheme turns into e: H(m), and H(Z || m) for SM2"""
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_verify_batch(self.ctx.h, self.h, alg, n, pubs, sigs, digests, hlen, res), "ec_sig_verify_batch")
        return res.raw[:n]

    def sig_sign(self, alg, privs, nonces, digests, hlen):
        """ECGDSA / ECRDSA / SM2 signatures (r || s) with caller-supplied nonces, and a status byte per item"""
        n = len(privs) // self.qlen
        sigs = C.create_string_buffer(max(1, 2 * self.qlen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_sign_batch(self.ctx.h, self.h, alg, n, privs, nonces, digests, hlen, sigs, st), "ec_sig_sign_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def sig_verify_msg(self, alg, hash_type, pubs, sigs, slots, stride, ident=None):
        """ECGDSA / ECRDSA / SM2 verification from message slots, hashed on the device (hash_type 1 .. 4, 11 SM3, 13 / 14 Streebog);
        SM2: `ident` is the signer's id of Z and every slot starts with a blank of the digest size"""
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_verify_msg_batch(self.ctx.h, self.h, alg, hash_type, n, pubs, sigs, slots, stride, ident,
                                                    len(ident) if ident else 0, res), "ec_sig_verify_msg_batch")
        return res.raw[:n]

    def sig_sign_msg(self, alg, hash_type, privs, nonces, slots, stride, ident=None, pubs=None):
        """ECGDSA / ECRDSA / SM2 signatures from message slots; SM2: pubs (for Z) may be None, then Y = [x]G on the device"""
        n = len(privs) // self.qlen
        sigs = C.create_string_buffer(max(1, 2 * self.qlen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_sign_msg_batch(self.ctx.h, self.h, alg, hash_type, n, privs, pubs, nonces, slots, stride, ident,
                                                  len(ident) if ident else 0, sigs, st), "ec_sig_sign_msg_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def sig_hashed_rlen(self, alg, hash_type):
        """bytes of r in a signature of ECSDSA / ECOSDSA (the digest size) or ECKCDSA (min(digest size, qlen))"""
        hs = HASH_SIZES.get(hash_type, 0)
        return min(hs, self.qlen) if alg == SIG_ECKCDSA else hs

    def sig_hashed_verify(self, alg, hash_type, pubs, sigs, inputs, stride):
        """ECSDSA / ECOSDSA / ECKCDSA verification: 0 accept / 1 reject per item.  inputs: message slots of `stride` bytes with the blank
        for the commitment in front of the message (ECSDSA, ECOSDSA), or the digests H(z || m) with stride = digest size (ECKCDSA)"""
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_hashed_verify_batch(self.ctx.h, self.h, alg, hash_type, n, pubs, sigs, inputs, stride, res),
             "ec_sig_hashed_verify_batch")
        return res.raw[:n]

    def sig_hashed_sign(self, alg, hash_type, privs, nonces, inputs, stride):
        """ECSDSA / ECOSDSA / ECKCDSA signatures (r || s) with caller-supplied nonces, and a status byte per item"""
        n = len(privs) // self.qlen
        sl = self.sig_hashed_rlen(alg, hash_type) + self.qlen
        sigs = C.create_string_buffer(max(1, sl * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_hashed_sign_batch(self.ctx.h, self.h, alg, hash_type, n, privs, nonces, inputs, stride, sigs, st),
             "ec_sig_hashed_sign_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def bign_siglen(self):
        """bytes of a BIGN signature: s0 (qlen // 2) then s1 (qlen), both little-endian"""
        return self.qlen // 2 + self.qlen

    def bign_verify(self, alg, hash_type, pubs, sigs, inputs, stride, oid):
        """BIGN / DBIGN verification (alg: SIG_BIGN, SIG_DBIGN): 0 accept / 1 reject per item.  hash_type 0: inputs are the digests
        H(m), stride their length; hash_type 1 .. 4 or HASH_BELT: inputs are message slots of `stride` bytes, hashed on the device.
        oid: the OID octets of the message's hash (at most 64)"""
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bign_verify_batch(self.ctx.h, self.h, alg, hash_type, n, pubs, sigs, inputs, stride, oid, len(oid), res),
             "ec_bign_verify_batch")
        return res.raw[:n]

    def bign_sign(self, alg, hash_type, privs, nonces, inputs, stride, oid):
        """BIGN / DBIGN signatures (s0 || s1, little-endian) with caller-supplied nonces (big-endian, like privs), and a status byte
        per item"""
        n = len(privs) // self.qlen
        sl = self.bign_siglen()
        sigs = C.create_string_buffer(max(1, sl * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bign_sign_batch(self.ctx.h, self.h, alg, hash_type, n, privs, nonces, inputs, stride, oid, len(oid), sigs, st),
             "ec_bign_sign_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def schnorr_rlen(self, alg):
        """bytes of the commitment in a BIP0340 (R.x) / ECFSDSA (W.x || W.y) signature"""
        return self.clen if alg == SIG_BIP0340 else 2 * self.clen

    def schnorr_verify(self, alg, hash_type, keys, key_fmt, sigs, slots, stride):
        """BIP0340 / ECFSDSA verification item by item (alg: SIG_BIP0340, SIG_ECFSDSA; hash_type 1 .. 4): 0 accept / 1 reject per item.
        keys: X || Y (key_fmt 0) or X || Y || Z (1); slots: the hash inputs of ec_schnorr_verify_msg_all_batch"""
        n = len(sigs) // (self.schnorr_rlen(alg) + self.qlen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_schnorr_verify_batch(self.ctx.h, self.h, alg, hash_type, n, keys, key_fmt, sigs, slots, stride, res),
             "ec_schnorr_verify_batch")
        return res.raw[:n]

    def schnorr_sign(self, alg, hash_type, privs, pubs, nonces, slots, stride):
        """BIP0340 / ECFSDSA signatures (r || s) with caller-supplied nonces, and a status byte per item; pubs: X || Y per item, or None
        (BIP0340 derives Y = [x]G on the device; ECFSDSA ignores it)"""
        n = len(privs) // self.qlen
        sl = self.schnorr_rlen(alg) + self.qlen
        sigs = C.create_string_buffer(max(1, sl * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_schnorr_sign_batch(self.ctx.h, self.h, alg, hash_type, n, privs, pubs, nonces, slots, stride, sigs, st),
             "ec_schnorr_sign_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def random_mod(self, raw):
        """nn_get_random_mod given its 2 * qlen random bytes per item: LE(raw) mod (q - 1) + 1, big-endian"""
        n = len(raw) // (2 * self.qlen)
        out = C.create_string_buffer(max(1, self.qlen * n))
        _chk(self.L, self.L.ec_nn_random_mod_batch(self.ctx.h, self.h, n, raw, out), "ec_nn_random_mod_batch")
        return out.raw[:self.qlen * n]

    def ecdsa_sign_msgs(self, privs, nonce_raw, hash_type, msgs, stride=None):
        """ECDSA signatures with the nonces reduced (nn_get_random_mod) and the messages hashed on the device; hash_type 0: msgs
        are digests of equal length"""
        n = len(privs) // self.qlen
        if hash_type:
            slots, stride = self.msg_slots(msgs, stride)
        else:
            slots, stride = b"".join(msgs), (len(msgs[0]) if msgs else 32)
        sigs, st = C.create_string_buffer(max(1, 2 * self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_sign_msg_batch(self.ctx.h, self.h, n, privs, nonce_raw, hash_type, slots, stride, sigs, st),
             "ec_ecdsa_sign_msg_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def rfc6979_nonce(self, hash_type, privs, digests):
        """the nonces of deterministic ECDSA (RFC 6979 section 3.2, HMAC over SHA-2 hash_type 1 .. 4) derived on the device:
        (n x qlen big-endian, status)"""
        n = len(privs) // self.qlen
        out, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_rfc6979_nonce_batch(self.ctx.h, self.h, hash_type, n, privs, digests, out, st), "ec_rfc6979_nonce_batch")
        return out.raw[:self.qlen * n], st.raw[:n]

    def decdsa_sign(self, hash_type, privs, inputs, stride, is_digest):
        """deterministic ECDSA signatures (r || s) and a status byte per item; inputs: message slots of `stride` bytes (is_digest
        False, hashed on the device) or the digests themselves (is_digest True, stride = the digest length)"""
        n = len(privs) // self.qlen
        sigs, st = C.create_string_buffer(max(1, 2 * self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_decdsa_sign_batch(self.ctx.h, self.h, hash_type, n, privs, inputs, stride, 1 if is_digest else 0, sigs, st),
             "ec_decdsa_sign_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def ecdsa_verify_msg_list(self, hash_type, pubs, sigs, msgs):
        """(ecdsa_verify_msgs is the older call over equal-length messages in slots and keeps its name.)  ECDSA verification of a list of `bytes` of any lengths, hashed on the device with any hash of DIGEST_SIZES: n result bytes"""
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecdsa_verify_msgs_batch(self.ctx.h, self.h, hash_type, n, pubs, sigs, packed, offs, res), "ec_ecdsa_verify_msgs_batch")
        return res.raw[:n]

    def decdsa_sign_msgs(self, hash_type, privs, msgs):
        """decdsa_sign_ht over a list of `bytes` of any lengths: (n x 2 qlen signature bytes, n status bytes)"""
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        sigs, st = C.create_string_buffer(max(1, 2 * self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_decdsa_sign_msgs_batch(self.ctx.h, self.h, hash_type, n, privs, packed, offs, sigs, st), "ec_decdsa_sign_msgs_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def rfc6979_nonce_ht(self, hash_type, privs, digests):
        """rfc6979_nonce with HMAC over any hash of DIGEST_SIZES (digests: n x DIGEST_SIZES[hash_type])"""
        n = len(privs) // self.qlen
        out, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_rfc6979_nonce_ht_batch(self.ctx.h, self.h, hash_type, n, privs, digests, out, st), "ec_rfc6979_nonce_ht_batch")
        return out.raw[:self.qlen * n], st.raw[:n]

    def decdsa_sign_ht(self, hash_type, privs, inputs, stride, is_digest):
        """decdsa_sign with any hash of DIGEST_SIZES as the message hash and the HMAC's hash"""
        n = len(privs) // self.qlen
        sigs, st = C.create_string_buffer(max(1, 2 * self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_decdsa_sign_ht_batch(self.ctx.h, self.h, hash_type, n, privs, inputs, stride, 1 if is_digest else 0, sigs, st),
             "ec_decdsa_sign_ht_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def dbign_nonce(self, privs, digests, digest_len, oid, t=b""):
        """the nonces of deterministic BIGN (STB 34.101.45 section 6.3.3) derived on the device from the digests of the messages
        (digest_len octets each), the OID of their hash and the optional additional data t: (n x qlen big-endian, status)"""
        n = len(privs) // self.qlen
        out, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_dbign_nonce_batch(self.ctx.h, self.h, n, privs, digests, digest_len, oid, len(oid), t, len(t), out, st),
             "ec_dbign_nonce_batch")
        return out.raw[:self.qlen * n], st.raw[:n]

    def dbign_sign(self, hash_type, privs, inputs, stride, oid, t=b""):
        """deterministic BIGN signatures (s0 || s1, little-endian) and a status byte per item, the nonce derived on the device;
        hash_type, inputs, stride and oid as for bign_sign"""
        n = len(privs) // self.qlen
        sl = self.bign_siglen()
        sigs, st = C.create_string_buffer(max(1, sl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_dbign_sign_batch(self.ctx.h, self.h, hash_type, n, privs, inputs, stride, oid, len(oid), t, len(t), sigs, st),
             "ec_dbign_sign_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def bip0340_nonce(self, hash_type, privs, pubs, aux, slots, stride):
        """BIP0340's nonces derived on the device from the keys, the aux values (n x qlen big-endian) and the signing slots of
        schnorr_sign; pubs: X || Y per item, or None (Y = [x]G on the device): (n x qlen big-endian, status)"""
        n = len(privs) // self.qlen
        out, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bip0340_nonce_batch(self.ctx.h, self.h, hash_type, n, privs, pubs, aux, slots, stride, out, st),
             "ec_bip0340_nonce_batch")
        return out.raw[:self.qlen * n], st.raw[:n]

    def bip0340_sign(self, hash_type, privs, pubs, aux, slots, stride):
        """BIP0340 signatures (r || s) and a status byte per item, the nonce derived on the device from the aux values"""
        n = len(privs) // self.qlen
        sl = self.clen + self.qlen
        sigs, st = C.create_string_buffer(max(1, sl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bip0340_sign_batch(self.ctx.h, self.h, hash_type, n, privs, pubs, aux, slots, stride, sigs, st),
             "ec_bip0340_sign_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def sig_hashed_rlen_ht(self, alg, hash_type):
        """Over the whole hash table (hash_type from DIGEST_SIZES): bytes of r in a signature of ECSDSA / ECOSDSA (the digest size) or ECKCDSA (min(digest size, qlen))"""
        hs = DIGEST_SIZES.get(hash_type, 0)
        return min(hs, self.qlen) if alg == SIG_ECKCDSA else hs

    def sig_hashed_verify_ht(self, alg, hash_type, pubs, sigs, inputs, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): ECSDSA / ECOSDSA / ECKCDSA verification: 0 accept / 1 reject per item.  inputs: message slots of `stride` bytes with the blank
        for the commitment in front of the message (ECSDSA, ECOSDSA), or the digests H(z || m) with stride = digest size (ECKCDSA)"""
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_hashed_verify_ht_batch(self.ctx.h, self.h, alg, hash_type, n, pubs, sigs, inputs, stride, res),
             "ec_sig_hashed_verify_ht_batch")
        return res.raw[:n]

    def sig_hashed_sign_ht(self, alg, hash_type, privs, nonces, inputs, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): ECSDSA / ECOSDSA / ECKCDSA signatures (r || s) with caller-supplied nonces, and a status byte per item"""
        n = len(privs) // self.qlen
        sl = self.sig_hashed_rlen_ht(alg, hash_type) + self.qlen
        sigs = C.create_string_buffer(max(1, sl * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_sig_hashed_sign_ht_batch(self.ctx.h, self.h, alg, hash_type, n, privs, nonces, inputs, stride, sigs, st),
             "ec_sig_hashed_sign_ht_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def schnorr_verify_ht(self, alg, hash_type, keys, key_fmt, sigs, slots, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): BIP0340 / ECFSDSA verification item by item (alg: SIG_BIP0340, SIG_ECFSDSA): 0 accept / 1 reject per item.
        keys: X || Y (key_fmt 0) or X || Y || Z (1); slots: the hash inputs of ec_schnorr_verify_msg_all_batch"""
        n = len(sigs) // (self.schnorr_rlen(alg) + self.qlen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_schnorr_verify_ht_batch(self.ctx.h, self.h, alg, hash_type, n, keys, key_fmt, sigs, slots, stride, res),
             "ec_schnorr_verify_ht_batch")
        return res.raw[:n]

    def schnorr_sign_ht(self, alg, hash_type, privs, pubs, nonces, slots, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): BIP0340 / ECFSDSA signatures (r || s) with caller-supplied nonces, and a status byte per item; pubs: X || Y per item, or None
        (BIP0340 derives Y = [x]G on the device; ECFSDSA ignores it)"""
        n = len(privs) // self.qlen
        sl = self.schnorr_rlen(alg) + self.qlen
        sigs = C.create_string_buffer(max(1, sl * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_schnorr_sign_ht_batch(self.ctx.h, self.h, alg, hash_type, n, privs, pubs, nonces, slots, stride, sigs, st),
             "ec_schnorr_sign_ht_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def bip0340_nonce_ht(self, hash_type, privs, pubs, aux, slots, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): BIP0340's nonces derived on the device from the keys, the aux values (n x qlen big-endian) and the signing slots of
        schnorr_sign; pubs: X || Y per item, or None (Y = [x]G on the device): (n x qlen big-endian, status)"""
        n = len(privs) // self.qlen
        out, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bip0340_nonce_ht_batch(self.ctx.h, self.h, hash_type, n, privs, pubs, aux, slots, stride, out, st),
             "ec_bip0340_nonce_ht_batch")
        return out.raw[:self.qlen * n], st.raw[:n]

    def bip0340_sign_ht(self, hash_type, privs, pubs, aux, slots, stride):
        """Over the whole hash table (hash_type from DIGEST_SIZES): BIP0340 signatures (r || s) and a status byte per item, the nonce derived on the device from the aux values"""
        n = len(privs) // self.qlen
        sl = self.clen + self.qlen
        sigs, st = C.create_string_buffer(max(1, sl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_bip0340_sign_ht_batch(self.ctx.h, self.h, hash_type, n, privs, pubs, aux, slots, stride, sigs, st),
             "ec_bip0340_sign_ht_batch")
        return sigs.raw[:sl * n], st.raw[:n]

    def key_pair_gen_raw(self, raw):
        """x = nn_get_random_mod value of the item's 2 * qlen random bytes, Y = [x]G: (privs, pubs affine, status)"""
        n = len(raw) // (2 * self.qlen)
        pr, pb, st = C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_key_pair_gen_raw_batch(self.ctx.h, self.h, n, raw, pr, pb, st), "ec_key_pair_gen_raw_batch")
        return pr.raw[:self.qlen * n], pb.raw[:2 * self.clen * n], st.raw[:n]

    def ecccdh(self, privs, peers):
        n = len(privs) // self.qlen
        sec = C.create_string_buffer(max(1, self.clen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_ecccdh_derive_batch(self.ctx.h, self.h, n, privs, peers, sec, st),
             "ec_ecccdh_derive_batch")
        return sec.raw[:self.clen * n], st.raw[:n]

    def xdh(self, k, u):
        """X25519 (WEI25519) / X448 (WEI448): little-endian scalars and u coordinates"""
        n = len(k) // self.clen
        out = C.create_string_buffer(max(1, self.clen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_xdh_batch(self.ctx.h, self.h, n, k, u, out, st), "ec_xdh_batch")
        return out.raw[:self.clen * n], st.raw[:n]

    def eddsa_verify(self, pubkeys, sigs, hram, hram_len=None):
        """Ed25519 (WEI25519 handle): 32-byte keys, 64-byte signatures, hram = SHA-512(dom2 || R || A || PH(M));
        Ed448 (WEI448 handle): 57-byte keys, 114-byte signatures, hram = SHAKE256(dom4 || R || A || PH(M), 114)"""
        klen = 57 if self.clen == 56 else self.clen
        hram_len = hram_len or (114 if self.clen == 56 else 64)
        n = len(pubkeys) // klen
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_verify_batch(self.ctx.h, self.h, n, pubkeys, sigs, hram, hram_len, res),
             "ec_eddsa_verify_batch")
        return res.raw[:n]

    def eddsa_sign_R(self, r_hash):
        """EdDSA signing, step 1: n x 64-byte SHA-512(dom2 || prefix || PH(M)) -> (n x 32 encoded R, status); on the WEI448
        handle n x 114-byte SHAKE256(dom4 || prefix || PH(M)) -> n x 57"""
        hl, kl = (114, 57) if self.clen == 56 else (64, 32)
        n = len(r_hash) // hl
        out, st = C.create_string_buffer(max(1, kl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_sign_R_batch(self.ctx.h, self.h, n, r_hash, out, st), "ec_eddsa_sign_R_batch")
        return out.raw[:kl * n], st.raw[:n]

    def eddsa_sign_S(self, r_hash, hram, a_scalars):
        """EdDSA signing, step 2: S = (r + hram * a) mod q, n x 32 (Ed25519) / n x 57 (Ed448) bytes little-endian"""
        hl, kl = (114, 57) if self.clen == 56 else (64, 32)
        n = len(r_hash) // hl
        out = C.create_string_buffer(max(1, kl * n))
        _chk(self.L, self.L.ec_eddsa_sign_S_batch(self.ctx.h, self.h, n, r_hash, hram, a_scalars, out), "ec_eddsa_sign_S_batch")
        return out.raw[:kl * n]

    def eddsa_sign_msgs(self, alg, secret_keys, pubkeys, adata, slots, stride, adata_len=None, want_pub=True):
        """one-call EdDSA signing with every hash on the device (alg: EDDSA25519 .. EDDSA448PH): secret_keys n x klen, pubkeys
        n x klen or None (derived on the device), adata the call's context (bytes or None), slots n message slots of `stride` bytes
        -> (sigs n x 2 klen, pub_out n x klen, status)"""
        kl = 57 if self.clen == 56 else 32
        n = len(secret_keys) // kl
        sigs, st = C.create_string_buffer(max(1, 2 * kl * n)), C.create_string_buffer(max(1, n))
        pub = C.create_string_buffer(max(1, kl * n)) if want_pub else None
        alen = (len(adata) if adata is not None else 0) if adata_len is None else adata_len
        _chk(self.L, self.L.ec_eddsa_sign_msg_batch(self.ctx.h, self.h, alg, n, secret_keys, pubkeys, adata, alen, slots, stride, sigs, pub, st),
             "ec_eddsa_sign_msg_batch")
        return sigs.raw[:2 * kl * n], (pub.raw[:kl * n] if want_pub else None), st.raw[:n]

    def eddsa_verify_msg_list(self, alg, pubkeys, sigs, msgs, adata=None):
        """(eddsa_verify_msgs is the older call over host-assembled hash inputs in slots and keeps its name.)  EdDSA verification of
        a list of `bytes` of any lengths, all five variants, every hash on the device: n result bytes"""
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_verify_msgs_batch(self.ctx.h, self.h, alg, n, pubkeys, sigs, adata, len(adata) if adata is not None else 0,
                                                       packed, offs, res), "ec_eddsa_verify_msgs_batch")
        return res.raw[:n]

    def eddsa_verify_msg_list_all(self, alg, pubkeys, sigs, msgs, adata=None):
        """ec_verify_batch's whole-batch predicate from the same inputs: (all_valid, index of the first rejected item or n)"""
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        ok, first = C.c_int(0), C.c_uint32(0)
        _chk(self.L, self.L.ec_eddsa_verify_msgs_all_batch(self.ctx.h, self.h, alg, n, pubkeys, sigs, adata, len(adata) if adata is not None else 0,
                                                           packed, offs, C.byref(ok), C.byref(first)), "ec_eddsa_verify_msgs_all_batch")
        return bool(ok.value), first.value

    def eddsa_sign_msg_list(self, alg, secret_keys, pubkeys, msgs, adata=None, want_pub=True):
        """eddsa_sign_msgs over a list of `bytes` of any lengths: (sigs n x 2 klen, pub_out n x klen or None, status)"""
        kl = 57 if self.clen == 56 else 32
        n = len(msgs)
        packed, offs = pack_msgs(msgs)
        sigs, st = C.create_string_buffer(max(1, 2 * kl * n)), C.create_string_buffer(max(1, n))
        pub = C.create_string_buffer(max(1, kl * n)) if want_pub else None
        _chk(self.L, self.L.ec_eddsa_sign_msgs_batch(self.ctx.h, self.h, alg, n, secret_keys, pubkeys, adata, len(adata) if adata is not None else 0,
                                                     packed, offs, sigs, pub, st), "ec_eddsa_sign_msgs_batch")
        return sigs.raw[:2 * kl * n], (pub.raw[:kl * n] if want_pub else None), st.raw[:n]

    def eddsa_pub_keys(self, secret_keys):
        """eddsa_import_key_pair_from_priv_key_buf + eddsa_export_pub_key in batch: (n x klen encodings of A, status)"""
        kl = 57 if self.clen == 56 else 32
        n = len(secret_keys) // kl
        pub, st = C.create_string_buffer(max(1, kl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_pub_key_batch(self.ctx.h, self.h, n, secret_keys, pub, st), "ec_eddsa_pub_key_batch")
        return pub.raw[:kl * n], st.raw[:n]

    def eddsa_encode_points(self, points_prj):
        """eddsa_export_pub_key in batch: projective Weierstrass X || Y || Z -> the 32 / 57-byte EdDSA encodings, status"""
        kl = 57 if self.clen == 56 else 32
        n = len(points_prj) // (3 * self.clen)
        out, st = C.create_string_buffer(max(1, kl * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_eddsa_encode_point_batch(self.ctx.h, self.h, n, points_prj, out, st), "ec_eddsa_encode_point_batch")
        return out.raw[:kl * n], st.raw[:n]

    def eddsa_verify_all(self, pubkeys, sigs, hram, hram_len=None):
        """ec_verify_batch's whole-batch predicate: (all_valid, index of the first rejected item or n)"""
        klen = 57 if self.clen == 56 else self.clen
        hram_len = hram_len or (114 if self.clen == 56 else 64)
        n = len(pubkeys) // klen
        ok, first = C.c_int(0), C.c_uint32(0)
        _chk(self.L, self.L.ec_eddsa_verify_all_batch(self.ctx.h, self.h, n, pubkeys, sigs, hram, hram_len,
                                                       C.byref(ok), C.byref(first)), "ec_eddsa_verify_all_batch")
        return bool(ok.value), first.value

    def debug_eddsa_msm(self, pubkeys, sigs, hram, seed):
        """test hook: (accept, z_i as n x 16 bytes little-endian, [X, Y, Z, T] of the sum before the cofactor as integers mod p)"""
        n = len(pubkeys) // 32
        acc = C.c_int(0)
        z = C.create_string_buffer(16 * n)
        w = (C.c_uint32 * 36)()
        _chk(self.L, self.L.ecamd_debug_eddsa_msm(self.ctx.h, self.h, n, pubkeys, sigs, hram, seed, C.byref(acc),
                                                   C.cast(z, C.c_void_p), C.cast(w, C.c_void_p)), "ecamd_debug_eddsa_msm")
        p = 2 ** 255 - 19
        coords = [sum(int(w[9 * c + i]) << (29 * i) for i in range(9)) % p for c in range(4)]
        return bool(acc.value), z.raw, coords

    def schnorr_verify_all(self, s, ne, keys_aff, r, r_fmt=0):
        """ec_schnorr_verify_all_batch: True iff sum z_i ([s_i]G + [ne_i]Y_i - R_i) vanishes (the BIP0340 / ECFSDSA batch equation as one
        multi-scalar multiplication); False = not decided here.  r_fmt 1: r holds x coordinates, R_i has the even y."""
        n = len(s) // self.qlen
        ok = C.c_int(0)
        _chk(self.L, self.L.ec_schnorr_verify_all_batch(self.ctx.h, self.h, n, s, ne, keys_aff, r, r_fmt, C.byref(ok)), "ec_schnorr_verify_all_batch")
        return bool(ok.value)

    def schnorr_msm_available(self, r_fmt=0):
        return bool(self.L.ec_schnorr_verify_all_available(self.h, r_fmt))

    def eddsa_verify_msg_prj_all(self, keys_prj, sigs, slots, stride, a_offset):
        """ec_eddsa_verify_msg_prj_all_batch: ec_verify_batch's one bit for plain Ed25519 from projective keys, signatures and hash inputs;
        True = the whole batch is valid, False = not decided here"""
        n = len(slots) // stride
        ok = C.c_int(0)
        _chk(self.L, self.L.ec_eddsa_verify_msg_prj_all_batch(self.ctx.h, self.h, n, keys_prj, sigs, slots, stride, a_offset, C.byref(ok)),
             "ec_eddsa_verify_msg_prj_all_batch")
        return bool(ok.value)

    def schnorr_verify_msg_all(self, keys, key_fmt, sigs, r_fmt, hash_type, slots, stride, x_offset):
        """ec_schnorr_verify_msg_all_batch: the BIP0340 / ECFSDSA batch from keys, signatures and hash inputs (hashes, q - e and the
        key's lift_x on the device); True = the whole batch is valid, False = not decided here"""
        n = len(slots) // stride
        ok = C.c_int(0)
        _chk(self.L, self.L.ec_schnorr_verify_msg_all_batch(self.ctx.h, self.h, n, keys, key_fmt, sigs, r_fmt, hash_type, slots, stride,
                                                             x_offset, C.byref(ok)), "ec_schnorr_verify_msg_all_batch")
        return bool(ok.value)

    def debug_schnorr_msm(self, s, ne, keys_aff, r, r_fmt, seed):
        """test hook: (accept, z_i as n x 16 bytes little-endian, the "sum is infinity" word of the lanes' sum)"""
        n = len(s) // self.qlen
        acc = C.c_int(0)
        z = C.create_string_buffer(16 * n)
        nw = self.L.ecamd_debug_schnorr_msm_words(self.h)
        w = (C.c_uint32 * max(1, nw))()
        _chk(self.L, self.L.ecamd_debug_schnorr_msm(self.ctx.h, self.h, n, s, ne, keys_aff, r, r_fmt, seed, C.byref(acc),
                                                     C.cast(z, C.c_void_p), C.cast(w, C.c_void_p)), "ecamd_debug_schnorr_msm")
        return bool(acc.value), z.raw, int(w[nw - 4]) if nw else None

    # -- device-pointer forms (torch tensors' data_ptr()); see include/libecc_amd.h for which ones synchronise --
    def eddsa_verify_all_dev(self, n, d_pubs, d_sigs, d_hram, d_verdict, stream=None):
        _chk(self.L, self.L.ec_eddsa_verify_all_batch_dev(self.ctx.h, self.h, n, d_pubs, d_sigs, d_hram, 114 if self.clen == 56 else 64, d_verdict, stream),
             "ec_eddsa_verify_all_batch_dev")

    def schnorr_verify_all_dev(self, n, d_s, d_ne, d_keys, d_r, r_fmt, d_verdict, stream=None):
        _chk(self.L, self.L.ec_schnorr_verify_all_batch_dev(self.ctx.h, self.h, n, d_s, d_ne, d_keys, d_r, r_fmt, d_verdict, stream),
             "ec_schnorr_verify_all_batch_dev")

    def ecdsa_verify_dev(self, n, d_pubs, d_sigs, d_digests, hlen, d_result, stream=None):
        _chk(self.L, self.L.ec_ecdsa_verify_batch_dev(self.ctx.h, self.h, n, d_pubs, d_sigs, d_digests, hlen, d_result,
                                                       stream), "ec_ecdsa_verify_batch_dev")

    def sig_verify_dev(self, alg, n, d_pubs, d_sigs, d_digests, hlen, d_result, stream=None):
        _chk(self.L, self.L.ec_sig_verify_batch_dev(self.ctx.h, self.h, alg, n, d_pubs, d_sigs, d_digests, hlen, d_result, stream),
             "ec_sig_verify_batch_dev")

    def sig_verify_msg_dev(self, alg, hash_type, n, d_pubs, d_sigs, d_slots, stride, ident, d_result, stream=None):
        _chk(self.L, self.L.ec_sig_verify_msg_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_pubs, d_sigs, d_slots, stride, ident,
                                                        len(ident) if ident else 0, d_result, stream), "ec_sig_verify_msg_batch_dev")

    def sig_sign_msg_dev(self, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, ident, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_sig_sign_msg_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, ident,
                                                      len(ident) if ident else 0, d_sigs, d_status, stream), "ec_sig_sign_msg_batch_dev")

    def sig_sign_dev(self, alg, n, d_privs, d_nonces, d_digests, hlen, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_sig_sign_batch_dev(self.ctx.h, self.h, alg, n, d_privs, d_nonces, d_digests, hlen, d_sigs, d_status,
                                                   stream), "ec_sig_sign_batch_dev")

    def sig_hashed_verify_dev(self, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, d_result, stream=None):
        _chk(self.L, self.L.ec_sig_hashed_verify_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, d_result,
                                                            stream), "ec_sig_hashed_verify_batch_dev")

    def bign_verify_dev(self, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, oid, d_result, stream=None):
        _chk(self.L, self.L.ec_bign_verify_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, oid, len(oid),
                                                      d_result, stream), "ec_bign_verify_batch_dev")

    def bign_sign_dev(self, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, oid, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_bign_sign_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, oid, len(oid),
                                                    d_sigs, d_status, stream), "ec_bign_sign_batch_dev")

    def sig_hashed_sign_dev(self, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_sig_hashed_sign_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, d_sigs,
                                                          d_status, stream), "ec_sig_hashed_sign_batch_dev")

    def schnorr_verify_dev(self, alg, hash_type, n, d_keys, key_fmt, d_sigs, d_slots, stride, d_result, stream=None):
        _chk(self.L, self.L.ec_schnorr_verify_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_keys, key_fmt, d_sigs, d_slots, stride, d_result,
                                                         stream), "ec_schnorr_verify_batch_dev")

    def schnorr_sign_dev(self, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_schnorr_sign_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, d_sigs,
                                                       d_status, stream), "ec_schnorr_sign_batch_dev")

    def ecdsa_recover_dev(self, n, d_sigs, d_digests, hlen, d_pub1, d_pub2, d_st1, d_st2, stream=None):
        _chk(self.L, self.L.ec_ecdsa_recover_batch_dev(self.ctx.h, self.h, n, d_sigs, d_digests, hlen, d_pub1, d_pub2, d_st1,
                                                        d_st2, stream), "ec_ecdsa_recover_batch_dev")

    def eddsa_verify_dev(self, n, d_pubs, d_sigs, d_hram, d_result, stream=None, hram_len=64):
        _chk(self.L, self.L.ec_eddsa_verify_batch_dev(self.ctx.h, self.h, n, d_pubs, d_sigs, d_hram, hram_len, d_result,
                                                       stream), "ec_eddsa_verify_batch_dev")

    def ecdsa_sign_dev(self, n, d_privs, d_nonces, d_digests, hlen, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_ecdsa_sign_batch_dev(self.ctx.h, self.h, n, d_privs, d_nonces, d_digests, hlen, d_sigs,
                                                     d_status, stream), "ec_ecdsa_sign_batch_dev")

    def rfc6979_nonce_dev(self, hash_type, n, d_privs, d_digests, d_nonces, d_status, stream=None):
        _chk(self.L, self.L.ec_rfc6979_nonce_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_digests, d_nonces, d_status, stream),
             "ec_rfc6979_nonce_batch_dev")

    def eddsa_sign_msgs_dev(self, alg, n, d_secret_keys, d_pubkeys, adata, d_slots, stride, d_sigs, d_pub_out, d_status, stream=None):
        """ec_eddsa_sign_msg_batch with device pointers (adata: host bytes or None; d_pubkeys, d_pub_out: a pointer or None)"""
        _chk(self.L, self.L.ec_eddsa_sign_msg_batch_dev(self.ctx.h, self.h, alg, n, d_secret_keys, d_pubkeys, adata,
                                                         len(adata) if adata is not None else 0, d_slots, stride, d_sigs, d_pub_out, d_status,
                                                         stream), "ec_eddsa_sign_msg_batch_dev")

    def eddsa_verify_msg_list_dev(self, alg, n, d_pubs, d_sigs, adata, d_msgs, msgs_len, d_offsets, d_result, stream=None):
        """ec_eddsa_verify_msgs_batch with device pointers (adata: host bytes or None)"""
        _chk(self.L, self.L.ec_eddsa_verify_msgs_batch_dev(self.ctx.h, self.h, alg, n, d_pubs, d_sigs, adata, len(adata) if adata is not None else 0,
                                                           d_msgs, msgs_len, d_offsets, d_result, stream), "ec_eddsa_verify_msgs_batch_dev")

    def eddsa_verify_msg_list_all_dev(self, alg, n, d_pubs, d_sigs, adata, d_msgs, msgs_len, d_offsets, d_all_valid, stream=None):
        """ec_eddsa_verify_msgs_all_batch with device pointers: d_all_valid[0] = 1 / 0"""
        _chk(self.L, self.L.ec_eddsa_verify_msgs_all_batch_dev(self.ctx.h, self.h, alg, n, d_pubs, d_sigs, adata, len(adata) if adata is not None else 0,
                                                               d_msgs, msgs_len, d_offsets, d_all_valid, stream), "ec_eddsa_verify_msgs_all_batch_dev")

    def eddsa_sign_msg_list_dev(self, alg, n, d_secret_keys, d_pubkeys, adata, d_msgs, msgs_len, d_offsets, d_sigs, d_pub_out, d_status, stream=None):
        """ec_eddsa_sign_msgs_batch with device pointers (d_pubkeys, d_pub_out: a pointer or None)"""
        _chk(self.L, self.L.ec_eddsa_sign_msgs_batch_dev(self.ctx.h, self.h, alg, n, d_secret_keys, d_pubkeys, adata, len(adata) if adata is not None else 0,
                                                         d_msgs, msgs_len, d_offsets, d_sigs, d_pub_out, d_status, stream), "ec_eddsa_sign_msgs_batch_dev")

    def eddsa_pub_keys_dev(self, n, d_secret_keys, d_pub_out, d_status, stream=None):
        _chk(self.L, self.L.ec_eddsa_pub_key_batch_dev(self.ctx.h, self.h, n, d_secret_keys, d_pub_out, d_status, stream),
             "ec_eddsa_pub_key_batch_dev")

    def decdsa_sign_dev(self, hash_type, n, d_privs, d_in, stride, is_digest, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_decdsa_sign_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_in, stride, 1 if is_digest else 0, d_sigs,
                                                      d_status, stream), "ec_decdsa_sign_batch_dev")

    def rfc6979_nonce_ht_dev(self, hash_type, n, d_privs, d_digests, d_nonces, d_status, stream=None):
        _chk(self.L, self.L.ec_rfc6979_nonce_ht_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_digests, d_nonces, d_status, stream),
             "ec_rfc6979_nonce_ht_batch_dev")

    def ecdsa_verify_msgs_dev(self, hash_type, n, d_pubs, d_sigs, d_msgs, msgs_len, d_offsets, d_result, stream=None):
        _chk(self.L, self.L.ec_ecdsa_verify_msgs_batch_dev(self.ctx.h, self.h, hash_type, n, d_pubs, d_sigs, d_msgs, msgs_len, d_offsets, d_result,
                                                           stream), "ec_ecdsa_verify_msgs_batch_dev")

    def decdsa_sign_msgs_dev(self, hash_type, n, d_privs, d_msgs, msgs_len, d_offsets, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_decdsa_sign_msgs_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_msgs, msgs_len, d_offsets, d_sigs, d_status,
                                                          stream), "ec_decdsa_sign_msgs_batch_dev")

    def decdsa_sign_ht_dev(self, hash_type, n, d_privs, d_in, stride, is_digest, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_decdsa_sign_ht_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_in, stride, 1 if is_digest else 0, d_sigs,
                                                         d_status, stream), "ec_decdsa_sign_ht_batch_dev")

    def dbign_nonce_dev(self, n, d_privs, d_digests, digest_len, oid, t, d_nonces, d_status, stream=None):
        _chk(self.L, self.L.ec_dbign_nonce_batch_dev(self.ctx.h, self.h, n, d_privs, d_digests, digest_len, oid, len(oid), t, len(t), d_nonces,
                                                      d_status, stream), "ec_dbign_nonce_batch_dev")

    def dbign_sign_dev(self, hash_type, n, d_privs, d_inputs, stride, oid, t, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_dbign_sign_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_inputs, stride, oid, len(oid), t, len(t), d_sigs,
                                                     d_status, stream), "ec_dbign_sign_batch_dev")

    def bip0340_nonce_dev(self, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_nonces, d_status, stream=None):
        _chk(self.L, self.L.ec_bip0340_nonce_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_nonces,
                                                        d_status, stream), "ec_bip0340_nonce_batch_dev")

    def bip0340_sign_dev(self, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_bip0340_sign_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_sigs,
                                                       d_status, stream), "ec_bip0340_sign_batch_dev")

    def sig_hashed_verify_ht_dev(self, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, d_result, stream=None):
        _chk(self.L, self.L.ec_sig_hashed_verify_ht_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_pubs, d_sigs, d_inputs, stride, d_result,
                                                            stream), "ec_sig_hashed_verify_ht_batch_dev")

    def sig_hashed_sign_ht_dev(self, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_sig_hashed_sign_ht_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_nonces, d_inputs, stride, d_sigs,
                                                          d_status, stream), "ec_sig_hashed_sign_ht_batch_dev")

    def schnorr_verify_ht_dev(self, alg, hash_type, n, d_keys, key_fmt, d_sigs, d_slots, stride, d_result, stream=None):
        _chk(self.L, self.L.ec_schnorr_verify_ht_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_keys, key_fmt, d_sigs, d_slots, stride, d_result,
                                                         stream), "ec_schnorr_verify_ht_batch_dev")

    def schnorr_sign_ht_dev(self, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_schnorr_sign_ht_batch_dev(self.ctx.h, self.h, alg, hash_type, n, d_privs, d_pubs, d_nonces, d_slots, stride, d_sigs,
                                                       d_status, stream), "ec_schnorr_sign_ht_batch_dev")

    def bip0340_nonce_ht_dev(self, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_nonces, d_status, stream=None):
        _chk(self.L, self.L.ec_bip0340_nonce_ht_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_nonces,
                                                        d_status, stream), "ec_bip0340_nonce_ht_batch_dev")

    def bip0340_sign_ht_dev(self, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_sigs, d_status, stream=None):
        _chk(self.L, self.L.ec_bip0340_sign_ht_batch_dev(self.ctx.h, self.h, hash_type, n, d_privs, d_pubs, d_aux, d_slots, stride, d_sigs,
                                                       d_status, stream), "ec_bip0340_sign_ht_batch_dev")

    def ecccdh_dev(self, n, d_privs, d_peers, d_secrets, d_status, stream=None):
        _chk(self.L, self.L.ec_ecccdh_derive_batch_dev(self.ctx.h, self.h, n, d_privs, d_peers, d_secrets, d_status,
                                                        stream), "ec_ecccdh_derive_batch_dev")

    def xdh_dev(self, n, d_k, d_u, d_out, d_status, stream=None):
        _chk(self.L, self.L.ec_xdh_batch_dev(self.ctx.h, self.h, n, d_k, d_u, d_out, d_status, stream),
             "ec_xdh_batch_dev")

    # -- point wire formats: 0 affine X || Y, 1 projective X || Y || Z --
    def scalar_mult_fmt(self, scalars, points, in_fmt, out_fmt, slen=None):
        slen = slen or self.qlen
        n = len(scalars) // slen
        w = (3 if out_fmt else 2) * self.clen
        out, st = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_mul_batch_fmt(self.ctx.h, self.h, n, scalars, slen, points, in_fmt, out, out_fmt, st),
             "ec_prj_pt_mul_batch_fmt")
        return out.raw[:w * n], st.raw[:n]

    def unique(self, points, in_fmt, out_fmt):
        n = len(points) // ((3 if in_fmt else 2) * self.clen)
        w = (3 if out_fmt else 2) * self.clen
        out, st = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_unique_batch(self.ctx.h, self.h, n, points, in_fmt, out, out_fmt, st),
             "ec_prj_pt_unique_batch")
        return out.raw[:w * n], st.raw[:n]

    def pt_op_fmt(self, op, p1, p2, in_fmt, out_fmt):
        """prj_pt_add (op 0) / prj_pt_dbl (1) / prj_pt_is_on_curve (2) / prj_pt_neg (3) in either wire format, prj_pt_cmp (4) /
        prj_pt_eq_or_opp (5) with one predicate byte per item: (out, status)"""
        iw, ow = (3 if in_fmt else 2) * self.clen, (1 if op >= 4 else (3 if out_fmt else 2) * self.clen)
        n = len(p1) // iw
        out, st = C.create_string_buffer(max(1, ow * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_op_batch_fmt(self.ctx.h, self.h, op, n, p1, p2, in_fmt, None if op == 2 else out, out_fmt, st),
             "ec_prj_pt_op_batch_fmt")
        return (b"" if op == 2 else out.raw[:ow * n]), st.raw[:n]

    def unprotected_mult(self, scalars, slen, points, in_fmt, out_fmt, broadcast=False):
        """_prj_pt_unprotected_mult per item (broadcast: one scalar of slen bytes for every point, check_prj_pt_order's use)"""
        iw, ow = (3 if in_fmt else 2) * self.clen, (3 if out_fmt else 2) * self.clen
        n = len(points) // iw
        out, st = C.create_string_buffer(max(1, ow * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_prj_pt_unprotected_mult_batch(self.ctx.h, self.h, n, scalars, slen, 0 if broadcast else slen, points, in_fmt,
                                                             out, out_fmt, st), "ec_prj_pt_unprotected_mult_batch")
        return out.raw[:ow * n], st.raw[:n]

    def y_from_x(self, xs):
        """aff_pt_y_from_x: (y1, y2, status), y1 the root the reference's fp_sqrt returns first"""
        n = len(xs) // self.clen
        y1, y2 = C.create_string_buffer(max(1, self.clen * n)), C.create_string_buffer(max(1, self.clen * n))
        st = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_aff_pt_y_from_x_batch(self.ctx.h, self.h, n, xs, y1, y2, st), "ec_aff_pt_y_from_x_batch")
        return y1.raw[:self.clen * n], y2.raw[:self.clen * n], st.raw[:n]

    def decompress(self, comp):
        """SEC 1 compressed points (0x02 / 0x03 || x) -> affine X || Y + status"""
        n = len(comp) // (self.clen + 1)
        out, st = C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_point_decompress_batch(self.ctx.h, self.h, n, comp, out, st), "ec_point_decompress_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]

    def structured_sigs(self, sigs, slen, alg_type, hash_type):
        n = len(sigs) // slen
        out, st = C.create_string_buffer(max(1, (slen - 3) * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_structured_sig_import_batch(self.h, n, sigs, slen, alg_type, hash_type, out, st),
             "ec_structured_sig_import_batch")
        return out.raw[:(slen - 3) * n], st.raw[:n]

    def structured_key_pairs(self, keys, klen, alg_type):
        """structured private keys -> (private scalars n x qlen, public keys X || Y || Z, status)"""
        n = len(keys) // klen
        pv, pb, st = (C.create_string_buffer(max(1, self.qlen * n)), C.create_string_buffer(max(1, 3 * self.clen * n)),
                      C.create_string_buffer(max(1, n)))
        _chk(self.L, self.L.ec_structured_key_pair_import_batch(self.ctx.h, self.h, n, keys, klen, alg_type, pv, pb, st),
             "ec_structured_key_pair_import_batch")
        return pv.raw[:self.qlen * n], pb.raw[:3 * self.clen * n], st.raw[:n]

    def structured_pub_keys(self, keys, alg_type):
        """libecc's structured public keys (3 header bytes + X || Y || Z) -> affine X || Y + status"""
        klen = 3 + 3 * self.clen
        n = len(keys) // klen
        out, st = C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ec_structured_pub_key_import_batch(self.ctx.h, self.h, n, keys, klen, alg_type, out, st),
             "ec_structured_pub_key_import_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]



class Multi:
    """ecamd_multi: one context and one host thread per listed device; batches are cut into contiguous shards.
    A device may be listed several times (its shards then share that GPU)."""

    def __init__(self, devices=None):
        self.L = load_library()
        self.h = C.c_void_p()
        if devices is None:
            rc = self.L.ecamd_multi_create(C.byref(self.h), None, 0)
        else:
            arr = (C.c_int * len(devices))(*devices)
            rc = self.L.ecamd_multi_create(C.byref(self.h), arr, len(devices))
        _chk(self.L, rc, "ecamd_multi_create")
        self.size = self.L.ecamd_multi_size(self.h)

    def close(self):
        if self.h:
            self.L.ecamd_multi_destroy(self.h)
            self.h = C.c_void_p()

    def shard_range(self, n, rank):
        lo, hi = C.c_uint32(0), C.c_uint32(0)
        self.L.ecamd_multi_shard_range(n, rank, self.size, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def curve(self, name):
        return MultiCurve(self, name)


class MultiCurve:
    def __init__(self, multi, name):
        self.m, self.L = multi, multi.L
        self.h = C.c_void_p()
        _chk(self.L, self.L.ecamd_multi_curve_by_name(multi.h, name.encode(), C.byref(self.h)), "ecamd_multi_curve_by_name")
        self.clen = self.L.ecamd_multi_curve_coord_len(self.h)
        self.qlen = self.L.ecamd_multi_curve_order_len(self.h)

    def free(self):
        if self.h:
            self.L.ecamd_multi_curve_free(self.h)
            self.h = C.c_void_p()

    def scalar_mult(self, scalars, points=None, slen=None):
        slen = slen or self.qlen
        n = len(scalars) // slen
        out, st = C.create_string_buffer(max(1, 2 * self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_prj_pt_mul_batch(self.m.h, self.h, n, scalars, slen, points, out, st),
             "ecamd_multi_prj_pt_mul_batch")
        return out.raw[:2 * self.clen * n], st.raw[:n]

    def ecdsa_verify(self, pubs, sigs, digests, hlen):
        n = len(pubs) // (2 * self.clen)
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_ecdsa_verify_batch(self.m.h, self.h, n, pubs, sigs, digests, hlen, res),
             "ecamd_multi_ecdsa_verify_batch")
        return res.raw[:n]

    def ecdsa_sign(self, privs, nonces, digests, hlen):
        n = len(privs) // self.qlen
        sigs, st = C.create_string_buffer(max(1, 2 * self.qlen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_ecdsa_sign_batch(self.m.h, self.h, n, privs, nonces, digests, hlen, sigs, st),
             "ecamd_multi_ecdsa_sign_batch")
        return sigs.raw[:2 * self.qlen * n], st.raw[:n]

    def ecccdh(self, privs, peers):
        n = len(privs) // self.qlen
        sec, st = C.create_string_buffer(max(1, self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_ecccdh_derive_batch(self.m.h, self.h, n, privs, peers, sec, st),
             "ecamd_multi_ecccdh_derive_batch")
        return sec.raw[:self.clen * n], st.raw[:n]

    def xdh(self, k, u):
        n = len(k) // self.clen
        out, st = C.create_string_buffer(max(1, self.clen * n)), C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_xdh_batch(self.m.h, self.h, n, k, u, out, st), "ecamd_multi_xdh_batch")
        return out.raw[:self.clen * n], st.raw[:n]

    def eddsa_verify(self, pubkeys, sigs, hram, hram_len=None):
        klen = 57 if self.clen == 56 else self.clen
        hram_len = hram_len or (114 if self.clen == 56 else 64)
        n = len(pubkeys) // klen
        res = C.create_string_buffer(max(1, n))
        _chk(self.L, self.L.ecamd_multi_eddsa_verify_batch(self.m.h, self.h, n, pubkeys, sigs, hram, hram_len, res),
             "ecamd_multi_eddsa_verify_batch")
        return res.raw[:n]

    def schnorr_verify_all(self, s, ne, keys_aff, r, r_fmt=0):
        n = len(s) // self.qlen
        ok = C.c_int(0)
        _chk(self.L, self.L.ecamd_multi_schnorr_verify_all_batch(self.m.h, self.h, n, s, ne, keys_aff, r, r_fmt, C.byref(ok)),
             "ecamd_multi_schnorr_verify_all_batch")
        return bool(ok.value)

    def eddsa_verify_all(self, pubkeys, sigs, hram, hram_len=None):
        klen = 57 if self.clen == 56 else self.clen
        hram_len = hram_len or (114 if self.clen == 56 else 64)
        n = len(pubkeys) // klen
        ok, first = C.c_int(0), C.c_uint32(0)
        _chk(self.L, self.L.ecamd_multi_eddsa_verify_all_batch(self.m.h, self.h, n, pubkeys, sigs, hram, hram_len,
                                                                C.byref(ok), C.byref(first)), "ecamd_multi_eddsa_verify_all_batch")
        return bool(ok.value), first.value
