"""ctypes binding of libpaintmind_hip.so (the C ABI declared in include/pmhip.h).

There is deliberately NO fallback: if the shared library is missing or a symbol cannot be resolved
the import of the compute path raises, and every op raises when handed a non-ROCm tensor.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpaintmind_hip.so")

PMHIP_OK = 0
PMHIP_EINVAL, PMHIP_EHIP, PMHIP_ENOMEM, PMHIP_ESTATE = 1, 2, 3, 4
F32, BF16 = 0, 1
PART_Q, PART_K, PART_V = 0, 1, 2
ABI_VERSION = 11
GENERATE_GRAPH, GENERATE_CONCURRENT_LANES, GENERATE_FROM_MASK = 1, 2, 4
SLOTS_GRAPH, SLOTS_KEEP_CONTEXT, SLOTS_KEEP_NEGATIVE = 1, 2, 4
GUIDE_OFF, GUIDE_UNCOND, GUIDE_NEGATIVE = 0, 1, 2   # SlotGuide.on: what a slot is guided against
SLOT_IDLE = 0x80000000             # bit 31 of Slot.step
CHOICE_T_MAX = 1000.0              # largest choice temperature of a step (include/pmhip.h, pmhip_remask_choice)

vp = C.c_void_p
i32 = C.c_int
f32 = C.c_float
u64 = C.c_uint64
u32 = C.c_uint32
i64 = C.c_int64


class LayerWeights(C.Structure):
    """mirror of pmhip_layer_weights"""
    _fields_ = [(n, vp) for n in (
        "ln1_g", "ln1_b", "wqkv", "wo", "bo", "lnx_g", "lnx_b", "wqkv2", "wo2", "bo2",
        "ln2_g", "ln2_b", "w12p", "b12p", "w3p", "b3",
        "wqkv_f", "qkv_c", "qkv_d", "wqkv2_f", "qkv2_c", "qkv2_d", "w12p_f", "w12_c", "w12_d")] + \
        [("bo_mean", C.c_float), ("bo2_mean", C.c_float), ("b3_mean", C.c_float)]


class TowerCfg(C.Structure):
    _fields_ = [("dim", i32), ("depth", i32), ("heads", i32), ("hidden_pad", i32), ("dim_head", i32)]


class VqganCfg(C.Structure):
    _fields_ = [("image_size", i32), ("patch_size", i32), ("channels", i32), ("n_embed", i32),
                ("embed_dim", i32), ("beta", f32), ("enc", TowerCfg), ("dec", TowerCfg)]


class VqganWeights(C.Structure):
    _fields_ = [("patch_w", vp), ("enc_pos", vp), ("pre_g", vp), ("pre_b", vp),
                ("enc_layers", C.POINTER(LayerWeights)), ("prevq_w", vp), ("prevq_b", vp),
                ("codebook_n", vp), ("codebook_sq", vp), ("postq_w", vp), ("postq_b", vp),
                ("dec_pos", vp), ("dec_layers", C.POINTER(LayerWeights)), ("dn_g", vp), ("dn_b", vp),
                ("proj_w", vp), ("proj_b", vp)]


class S2Cfg(C.Structure):
    _fields_ = [("tokens", i32), ("embed_dim", i32), ("n_embed", i32), ("context_dim", i32),
                ("context_dim_pad", i32), ("tower", TowerCfg)]


class S2Weights(C.Structure):
    _fields_ = [("tok_table", vp), ("tokproj_w", vp), ("tokproj_b", vp), ("pos", vp), ("ctxproj_w", vp),
                ("layers", C.POINTER(LayerWeights)), ("norm_g", vp), ("norm_b", vp), ("logits_w", vp),
                ("logits_b", vp), ("logits_wf", vp), ("logits_c", vp), ("logits_d", vp)]


class LnFold(C.Structure):
    """mirror of pmhip_lnfold"""
    _fields_ = [("coef", vp), ("c", vp), ("d", vp), ("parts", vp), ("nparts", i32), ("eps", f32)]


class Slot(C.Structure):
    """mirror of pmhip_slot: the decode state of one image of a batch (32 bytes)"""
    _fields_ = [("seed", u64), ("image_index", u64), ("temperature", f32), ("topk", i32), ("num_mask", i32), ("step", u32)]


class SlotGuide(C.Structure):
    """mirror of pmhip_slot_guide: the guidance of one image of a batch (8 bytes; on = 0: not guided, 1: against the pass without a
    context, 2: against the negative context)"""
    _fields_ = [("scale", f32), ("on", u32)]


# name -> (restype, argtypes); every symbol include/pmhip.h declares
PROTOTYPES = {
    "pmhip_abi_version": (i32, []),
    "pmhip_last_error": (C.c_char_p, []),
    "pmhip_device_info": (i32, [i32, C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32]),
    "pmhip_gemm": (i32, [i32, vp, i32, vp, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp]),
    "pmhip_gemm_swiglu": (i32, [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "pmhip_gemm_heads": (i32, [i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32),
                               C.POINTER(vp), f32, vp]),
    "pmhip_gemm_hilo": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp]),
    "pmhip_gemm_hilo_stats": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp]),
    "pmhip_gemm_hilo_center": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, C.c_float, vp, i32, vp]),
    "pmhip_unshift_hilo": (i32, [vp, vp, vp, i32, i32, vp]),
    "pmhip_ln_coef_parts": (i32, [vp, i32, f32, vp, i32, vp]),
    "pmhip_layernorm_hilo": (i32, [vp, vp, vp, vp, f32, vp, i32, i32, i32, vp]),
    "pmhip_layernorm_to_hilo": (i32, [vp, vp, vp, f32, vp, vp, i32, i32, vp]),
    "pmhip_split_hilo": (i32, [vp, vp, vp, i32, i32, vp]),
    "pmhip_join_hilo": (i32, [vp, vp, vp, i32, i32, vp]),
    "pmhip_ln_coef": (i32, [vp, f32, vp, i32, i32, vp]),
    "pmhip_gemm_ln": (i32, [i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, C.POINTER(LnFold), vp]),
    "pmhip_gemm_softmax_stats": (i32, [i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, C.POINTER(LnFold), vp, vp]),
    "pmhip_gemm_swiglu_ln": (i32, [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, C.POINTER(LnFold), vp]),
    "pmhip_gemm_heads_ln": (i32, [i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32),
                                  C.POINTER(vp), f32, C.POINTER(LnFold), vp]),
    "pmhip_lnfold_supported": (i32, [i32, i32, i32, i32, i32]),
    "pmhip_attention": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "pmhip_attention_fallbacks": (i32, [C.POINTER(C.c_ulonglong), i32]),
    "pmhip_gemm_heads_dh": (i32, [i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32),
                                  C.POINTER(vp), f32, vp, vp]),
    "pmhip_attention_dh": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "pmhip_attention_lens": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "pmhip_layernorm": (i32, [vp, vp, vp, f32, vp, i32, i32, i32, vp]),
    "pmhip_patchify": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "pmhip_unpatchify_clamp": (i32, [vp, vp, i32, i32, i32, i32, i32, f32, f32, vp]),
    "pmhip_convert_pad": (i32, [vp, i32, vp, i32, i32, i32, vp]),
    "pmhip_add_rows": (i32, [vp, vp, i32, vp, i32, i32, vp]),
    "pmhip_guidance_combine": (i32, [vp, vp, C.c_float, vp, C.c_size_t, vp]),
    "pmhip_guidance_combine_stats": (i32, [vp, vp, C.c_float, vp, C.c_size_t, vp, vp]),
    "pmhip_embed_rows": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "pmhip_random_mask": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp]),
    "pmhip_masked_ce": (i32, [vp, i32, vp, vp, f32, vp, vp, i32, i32, vp]),
    "pmhip_vq_prepare": (i32, [vp, vp, vp, i32, i32, vp]),
    "pmhip_vq_scratch_bytes": (C.c_size_t, [i32, i32]),
    "pmhip_vq_quantize": (i32, [vp, vp, vp, f32, vp, vp, vp, vp, i32, i32, i32, vp]),
    "pmhip_sample_rows": (i32, [vp, i32, vp, i64, i32, f32, vp, u64, u32, u64, vp, vp, vp, i32, i32, vp]),
    "pmhip_sample_rows_stats": (i32, [vp, i32, vp, vp, i64, i32, f32, vp, u64, u32, u64, vp, vp, vp, i32, i32, vp]),
    "pmhip_remask": (i32, [vp, vp, i32, i64, i32, i32, vp]),
    "pmhip_sample_rows_slots": (i32, [vp, i32, vp, vp, i64, vp, i32, vp, vp, vp, i32, i32, vp]),
    "pmhip_remask_slots": (i32, [vp, vp, vp, i64, i32, i32, vp]),
    "pmhip_pipeline_step_slots": (i32, [vp, vp, vp, i32, i32, C.POINTER(Slot), i32, vp, vp, vp]),
    "pmhip_guidance_combine_slots": (i32, [vp, vp, vp, vp, i32, vp, vp, i32, i32, vp]),
    "pmhip_pipeline_step_slots_guided": (i32, [vp, vp, vp, i32, i32, C.POINTER(Slot), C.POINTER(SlotGuide), i32, vp, vp, vp]),
    "pmhip_vqgan_create": (i32, [C.POINTER(vp), i32, i32, C.POINTER(VqganCfg), C.POINTER(VqganWeights)]),
    "pmhip_vqgan_destroy": (None, [vp]),
    "pmhip_vqgan_encode": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "pmhip_vqgan_decode": (i32, [vp, vp, i32, vp, vp]),
    "pmhip_vqgan_decode_indices": (i32, [vp, vp, i32, vp, vp]),
    "pmhip_vqgan_encoder_forward": (i32, [vp, vp, i32, vp, vp]),
    "pmhip_vqgan_decoder_forward": (i32, [vp, vp, i32, vp, vp]),
    "pmhip_s2_create": (i32, [C.POINTER(vp), i32, i32, C.POINTER(S2Cfg), C.POINTER(S2Weights)]),
    "pmhip_s2_destroy": (None, [vp]),
    "pmhip_s2_forward": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "pmhip_pipeline_sample": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, vp]),
    "pmhip_pipeline_generate": (i32, [vp, vp, vp, vp, i32, i32, i32, C.POINTER(f32), C.POINTER(i32),
                                      C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp]),
    "pmhip_pipeline_sample_guided": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, f32, vp]),
    "pmhip_pipeline_generate_guided": (i32, [vp, vp, vp, vp, i32, i32, i32, C.POINTER(f32), C.POINTER(i32),
                                             C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, f32]),
    "pmhip_s2_forward_lens": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), vp, vp]),
    "pmhip_pipeline_sample_lens": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32, vp]),
    "pmhip_pipeline_generate_lens": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                           C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32]),
    "pmhip_pipeline_step_slots_lens": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), i32, vp, vp, vp]),
    "pmhip_remask_choice": (i32, [vp, vp, i32, i64, i32, i32, f32, vp, u64, u32, u64, vp]),
    "pmhip_remask_choice_slots": (i32, [vp, vp, vp, vp, i64, i32, i32, vp]),
    "pmhip_pipeline_sample_choice": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32,
                                           f32, vp, vp]),
    "pmhip_pipeline_generate_choice": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                             C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32)]),
    "pmhip_pipeline_step_slots_choice": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                               i32, vp, vp, vp]),
    "pmhip_sample_rows_nucleus": (i32, [vp, i32, vp, i64, i32, f32, f32, vp, u64, u32, u64, vp, vp, vp, i32, i32, vp]),
    "pmhip_sample_rows_forced": (i32, [vp, i32, vp, vp, i64, vp, vp, vp, i32, i32, vp]),
    "pmhip_logit_divergence": (i32, [vp, vp, i32, vp, i64, i32, vp, vp, i32, i32, i32, vp]),
    "pmhip_token_logprob": (i32, [vp, vp, f32, i32, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "pmhip_pipeline_sample_nucleus": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32,
                                            f32, vp, f32, vp]),
    "pmhip_pipeline_generate_nucleus": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                              C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32),
                                              f32]),
    "pmhip_guidance_combine_dev": (i32, [vp, vp, vp, vp, C.c_size_t, vp, vp]),
    "pmhip_pipeline_sample_negative": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32,
                                             f32, vp, f32, vp, i32, C.POINTER(i32), vp]),
    "pmhip_pipeline_generate_negative": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                               C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32),
                                               f32, vp, i32, C.POINTER(i32), C.POINTER(f32)]),
    # the edit call: a re-masking count per image, the pixel-side operators, the edit loop
    "pmhip_remask_counts": (i32, [vp, vp, vp, i64, i32, i32, vp]),
    "pmhip_remask_choice_counts": (i32, [vp, vp, vp, i64, i32, i32, f32, vp, u64, u32, u64, vp]),
    "pmhip_mask_tokens": (i32, [vp, i32, vp, i64, vp, i32, i32, i32, vp]),
    "pmhip_composite": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "pmhip_pipeline_generate_edit": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                           C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32),
                                           f32, vp, i32, C.POINTER(i32), C.POINTER(f32)]),
    # regional prompts: the operator with a key set per query, and the model-level entries that take the
    # segment of every context row (host uint8 [B, L]) and the segments of every token (host uint32 [B, tokens])
    "pmhip_attention_segments": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "pmhip_s2_graph_count": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "pmhip_s2_forward_segments": (i32, [vp, vp, vp, i32, i32, C.POINTER(C.c_ubyte), C.POINTER(u32), vp, vp]),
    "pmhip_pipeline_sample_segments": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32,
                                             f32, vp, f32, vp, i32, C.POINTER(i32), C.POINTER(C.c_ubyte), C.POINTER(u32), vp]),
    "pmhip_pipeline_generate_segments": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                               C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32),
                                               f32, vp, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(C.c_ubyte), C.POINTER(u32)]),
    # prompt weights: the operator with a bias per key, the weights -> bias kernel, and the model-level entries
    # that take the weight of every context row (host f32 [B, L])
    "pmhip_attention_weighted": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "pmhip_key_bias": (i32, [vp, vp, i32, i32, vp]),
    "pmhip_s2_forward_weights": (i32, [vp, vp, vp, i32, i32, C.POINTER(C.c_ubyte), C.POINTER(u32), C.POINTER(f32), vp, vp]),
    "pmhip_pipeline_sample_weights": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, f32, i32, vp, u64, u32, u64, vp, vp, vp, i32, f32,
                                            f32, vp, f32, vp, i32, C.POINTER(i32), C.POINTER(C.c_ubyte), C.POINTER(u32), C.POINTER(f32), vp]),
    "pmhip_pipeline_generate_weights": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(i32), i32, C.POINTER(f32), C.POINTER(i32),
                                              C.POINTER(C.c_ubyte), i32, u64, u64, vp, i32, vp, vp, C.c_size_t, vp, i32, f32, C.POINTER(f32),
                                              f32, vp, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(C.c_ubyte), C.POINTER(u32),
                                              C.POINTER(f32)]),
    "pmhip_s2_switches": (i32, [vp]),
    "pmhip_vqgan_switches": (i32, [vp]),
    "pmhip_s2_step0_shared": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "pmhip_s2_slots_steps": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    # a negative prompt per slot: the combine of one kind of slot, the widest slots entry, its counters
    "pmhip_guidance_combine_slots_which": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp]),
    "pmhip_pipeline_step_slots_negative": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                                 vp, i32, C.POINTER(i32), i32, vp, vp, vp]),
    "pmhip_s2_slots_passes": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    # the sampler filters per slot: the operator with a launch per class, the slots entry that takes top-k up
    # to n_embed and a nucleus mass per slot, its counters
    "pmhip_sample_rows_slots_filter": (i32, [vp, i32, vp, vp, i64, vp, vp, i32, vp, vp, vp, i32, i32, vp]),
    "pmhip_pipeline_step_slots_filter": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                               vp, i32, C.POINTER(i32), C.POINTER(f32), i32, vp, vp, vp]),
    "pmhip_s2_slots_filter_steps": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
    "pmhip_remask_slots_counts": (i32, [vp, vp, vp, vp, i64, i32, i32, vp]),
    "pmhip_remask_choice_slots_counts": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, vp]),
    "pmhip_pipeline_step_slots_edit": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                             vp, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(i32), i32, vp, vp, vp]),
    "pmhip_s2_slots_edit_steps": (i32, [vp, C.POINTER(i32)]),
    # regional prompts per slot: the picked forms of the per-image and the per-query cross-attention, and the
    # slots step that runs one launch of each into one buffer
    "pmhip_attention_pick": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]),
    "pmhip_attention_pick_weighted": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]),
    "pmhip_pipeline_step_slots_regions": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                                vp, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(i32), C.POINTER(C.c_ubyte),
                                                C.POINTER(u32), C.POINTER(C.c_ubyte), i32, vp, vp, vp]),
    "pmhip_s2_slots_region_steps": (i32, [vp, C.POINTER(i32)]),
    "pmhip_pipeline_step_slots_weights": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(Slot), C.POINTER(SlotGuide), C.POINTER(f32),
                                                vp, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(i32), C.POINTER(C.c_ubyte),
                                                C.POINTER(u32), C.POINTER(C.c_ubyte), C.POINTER(f32), i32, vp, vp, vp]),
    "pmhip_s2_slots_weight_steps": (i32, [vp, C.POINTER(i32)]),
    # cross-attention maps: the operator, and the forward that taps chosen layers
    "pmhip_attention_maps": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, f32, i32, vp]),
    "pmhip_s2_forward_maps": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(C.c_ubyte), C.POINTER(u32), C.POINTER(f32), u64, vp, vp,
                                    vp]),
    # cross-attention control: the edited pass of a prompt-to-prompt pair, blended from the source pass
    "pmhip_attention_control": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "pmhip_s2_forward_control": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), u64, u64, C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), vp, vp]),
    # local blend: where a pair looks at a phrase, the region that follows, the token blend under it
    "pmhip_attention_phrase_score": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                           f32, i32, vp]),
    "pmhip_s2_forward_control_scores": (i32, [vp, vp, vp, i32, i32, C.POINTER(i32), u64, u64, C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), u64,
                                              C.POINTER(f32), C.POINTER(f32), vp, vp, i32, vp]),
    "pmhip_phrase_region": (i32, [vp, vp, vp, i32, i32, f32, i32, vp]),
    "pmhip_blend_tokens": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    # the Flan-T5 encoder's own operators: RMS norm, gated GELU, attention with the relative-position bias
    "pmhip_rmsnorm": (i32, [vp, vp, f32, vp, i32, i32, i32, vp]),
    "pmhip_geglu": (i32, [vp, i32, vp, i32, i32, i32, i32, vp]),
    "pmhip_attention_relbias": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    # the OpenCLIP text tower's own operators: causal attention, head split of a biased projection, the GELUs
    "pmhip_attention_causal": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "pmhip_split_heads": (i32, [i32, vp, i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(vp), f32, vp]),
    "pmhip_gelu": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, vp]),
    # canvases beyond the token grid: the fusion of window logits, the blend of decoded window pixels
    "pmhip_window_logits": (i32, [vp, vp, f32, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, vp]),
    "pmhip_window_pixels": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "pmhip_timing_enable": (i32, [i32]),
    "pmhip_timing_reset": (i32, []),
    "pmhip_timing_get": (i32, [C.c_char_p, C.POINTER(i32), C.POINTER(C.c_double)]),
}

_lib = None


class PmhipError(RuntimeError):
    pass


def load():
    """Load the library (once) and bind every prototype.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PmhipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (or paintmind_amd/csrc/build.sh). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.pmhip_abi_version()
    if got != ABI_VERSION:
        raise PmhipError(f"libpaintmind_hip.so ABI version {got} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != PMHIP_OK:
        msg = load().pmhip_last_error()
        err = PmhipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
        err.code = rc                     # a PMHIP_E* value
        raise err
