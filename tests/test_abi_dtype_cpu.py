"""The dtype check of the C-ABI, one launching entry point per csrc/*.hip source, without a GPU.

Every row's arguments pass each check that stands before the dtype check (non-null, 16-byte aligned pointers that are never
dereferenced; supported shapes), so dtype = 7 is the first thing wrong with the call: it must come back as STA_E_UNSUP with the
text below and must not reach a launch. The texts were recorded from the library as it was before the launches went through
sta_by_dtype / sta_launch (csrc/sta_internal.h): the refusal a caller reads must not depend on how the host side is written.
"""
import ctypes

import pytest

STA_E_UNSUP = -2
BAD_DTYPE = 7
P = 0x10000                                            # a fake device pointer: non-null, 16-byte aligned, never read
_BOX = (ctypes.c_int * 5)(0, 0, 64, 0, 64)             # sta_clip_views reads its boxes on the host (after the dtype check)
_BOX_PTR = ctypes.cast(_BOX, ctypes.c_void_p).value

# source -> (entry point, arguments up to the dtype, arguments behind it, text of sta_last_error())
TABLE = {
    "sta_xattn.hip": ("sta_xattn_pack_kv", (P, P, P, 1, 77, 320, 8), (0,), "dtype 7"),
    "sta_xattn_bwd.hip": ("sta_xattn_bwd", (P, P, 0, 0, P, P, 0, 0, 1, 256, 320, 8, 77, 0, 0.15), (0,), "dtype 7"),
    "sta_xattn_proj.hip": ("sta_xattn_pack_wq", (P, P, 320, 8), (0,), "dtype 7"),
    "sta_rowgemm.hip": ("sta_to_out_ln_pack_wo", (P, P, 320, 8, 0), (0,), "dtype 7"),
    "sta_ffgemm.hip": ("sta_ff_out_pack_w", (P, P, 320, 1280), (0,), "dtype 7"),
    "sta_lnqkv.hip": ("sta_ln_qkv_pack_w", (P, P, P, 320), (0,), "dtype 7"),
    "sta_conv.hip": ("sta_conv3x3_pack_w", (P, 576, 9, 3, 1, P, 64, 128), (0,), "dtype 7"),
    "sta_gemm.hip": ("sta_linear_rows_pack_w", (P, 64, 1, P, 64, 128), (0,), "dtype 7"),
    "sta_selfattn.hip": ("sta_selfattn_fwd", (P, P, P, P, 1, 64, 320, 8, 320, 320, 64, 64 * 320, 0.15), (0,), "dtype 7"),
    "sta_selfattn_bwd.hip": ("sta_selfattn_bwd", (P,) * 13 + (1, 64, 320, 8, 320, 320, 0.15), (0,), "dtype 7"),
    "sta_unet.hip": ("sta_geglu", (P, P, 4, 8), (0,), "dtype 7"),
    "sta_unet_bwd.hip": ("sta_geglu_bwd", (P, P, P, 4, 8), (0,), "dtype 7"),
    "sta_fp8.hip": ("sta_quant_rows_fp8", (P, P, P, 4, 64), (0,), "dtype 7"),
    "sta_mxfp8.hip": ("sta_mx8_quant_rows", (P, P, P, 4, 32), (0,), "dtype 7"),
    "sta_sampler.hip": ("sta_sampler_step", (P,) * 7 + (1, 8, 7.5, 0.5, 0.8, 1.0, 0.1, 0.0, 0.2, 0.0), (0,), "dtype 7"),
    "sta_encode.hip": ("sta_vae_encode_step", (P,) * 8 + (1, 64, 0.18215, 0.9, 0.4), (0,), "dtype 7"),
    "sta_clip.hip": ("sta_clip_views", (P, P, _BOX_PTR, P, 1, 256, 256, 1), (0,), "clip_views: dtype 7"),
    "sta_inpaint.hip": ("sta_latent_blend", (P,) * 6 + (1, 64, 64, 0.9, 0.4), (0,), "dtype 7"),
}
# sta_xattn_proj3.hip has no entry point of its own: its kernels are reached through sta_xattn_pack_kv_proj / sta_xattn_fwd_proj*
# (sta_xattn_proj.hip), which check the dtype before they call into it.
NO_DTYPE_ENTRY = {"sta_xattn_proj3.hip"}


def test_table_covers_every_source():
    import os
    from sta import lib
    assert set(TABLE) | NO_DTYPE_ENTRY == {os.path.basename(s) for s in lib.SOURCES}
    assert not set(TABLE) & NO_DTYPE_ENTRY


@pytest.mark.parametrize("source", sorted(TABLE))
def test_bad_dtype_is_refused_before_any_launch(source):
    from sta import lib
    L = lib.load()
    name, head, tail, text = TABLE[source]
    args = head + (BAD_DTYPE,) + tail
    assert len(args) == len(lib.SYMBOLS[name][1]), name
    rc = getattr(L, name)(*args)
    print(source, name, rc, L.sta_last_error())
    assert rc == STA_E_UNSUP, (name, rc, L.sta_last_error())
    assert L.sta_last_error().decode() == text, name
