"""Host code of the per-point FiLM family's mapping-network stage (cnerf_pfilm_backward_finish), no GPU: the exported symbols, the
sizes it asks for and what it refuses before any launch."""
import ctypes
import os

import pytest

SYMBOLS = ("cnerf_pfilm_finish_bytes", "cnerf_pack_pfilm_map_transposed", "cnerf_pfilm_backward_finish")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def stage_cfg(L, kinds=("pfilm",) * 8, precision="fp32", H=256):
    cfg = L.Cfg()
    cfg.B, cfg.V, cfg.C, cfg.H, cfg.L = 2, 16, 32, H, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = L.LAYER_CODE[k]
    cfg.voxel_length = 1.2
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, 16, 32
    cfg.precision = L.PREC_CODE[precision]
    return cfg                      # R, S, fov left at 0: the stage does not read them


def finish_bytes(L, cfg, n_images, n_per_image):
    pm, ws = ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.lib().cnerf_pfilm_finish_bytes(ctypes.byref(cfg), n_images, n_per_image, ctypes.byref(pm), ctypes.byref(ws))
    return rc, pm.value, ws.value


def finish(L, cfg, n_images=1, n_per_image=64, chunk=None, grads=True, ws=0x1000):
    """cnerf_pfilm_backward_finish with made-up, aligned, non-NULL addresses (never dereferenced on the host: a refusal launches nothing)."""
    p = ctypes.c_void_p
    chunk = [0x1000] * 6 if chunk is None else chunk          # packed_map, points, act_feat, act_h, act_g, act_go
    g = L.FieldParamGrads()
    return L.lib().cnerf_pfilm_backward_finish(ctypes.byref(cfg), None, p(chunk[0]), n_images, n_per_image, *(p(a) for a in chunk[1:]),
                                               ctypes.byref(g) if grads else None, None, None, p(ws), None)


def test_symbols_are_exported_and_prototyped(L):
    lib = L.lib()
    assert lib.cnerf_abi_version() == 10 == L.ABI_VERSION
    for name in SYMBOLS:
        assert name in L.PROTOTYPES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.PROTOTYPES[name][1]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cnerf.h")) as f:
        header = f.read()
    assert all(f"int {name}(" in header for name in SYMBOLS) and "#define CNERF_ABI_VERSION 10" in header


@pytest.mark.parametrize("H", [64, 128, 256])
def test_finish_bytes(L, H):
    cfg = stage_cfg(L, H=H)
    rc, pm, ws = finish_bytes(L, cfg, 2, 1000)
    assert rc == 0, L.lib().cnerf_last_error()
    assert pm >= 4 * (2 * 8 * H * 256 + 256 * 32)                 # both mapping matrices
    assert ws >= 4 * 2 * 1000 * (256 + 32)                        # g_mpre and d feat of every row
    assert finish_bytes(L, cfg, 3, 1000)[2] > ws and finish_bytes(L, cfg, 2, 1001)[2] > ws
    assert finish_bytes(L, cfg, 3, 1000)[1] == pm                 # the packed matrices do not depend on the chunk
    cfg.B = 64                                                    # nor does anything on the call's image count
    assert finish_bytes(L, cfg, 2, 1000) == (0, pm, ws)
    # outputs are optional
    assert L.lib().cnerf_pfilm_finish_bytes(ctypes.byref(cfg), 1, 1, None, None) == 0


def test_refusals_launch_nothing_and_say_why(L):
    err = lambda: L.lib().cnerf_last_error()
    assert finish_bytes(L, stage_cfg(L, kinds=("film",) * 4), 1, 64)[0] == -22 and b"per-point FiLM" in err()
    assert finish_bytes(L, stage_cfg(L, precision="fp16x3"), 1, 64)[0] == -22 and b"CNERF_PREC_FP32" in err()
    assert finish_bytes(L, stage_cfg(L), 0, 64)[0] == -22 and b"n_images" in err()
    assert finish_bytes(L, stage_cfg(L), 1, 0)[0] == -22 and err()
    # the call itself: the same refusals, then NULL chunk pointers, each before any launch
    assert finish(L, stage_cfg(L, kinds=("film",) * 4)) == -22 and b"per-point FiLM" in err()
    assert finish(L, stage_cfg(L, precision="fp16x3")) == -22 and b"CNERF_PREC_FP32" in err()
    assert finish(L, stage_cfg(L), n_images=0) == -22 and b"n_images" in err()
    for i in range(6):
        chunk = [0x1000] * 6
        chunk[i] = None
        assert finish(L, stage_cfg(L), chunk=chunk) == -22 and b"NULL" in err(), i
    assert finish(L, stage_cfg(L), grads=False) == -22 and b"NULL" in err()
    assert finish(L, stage_cfg(L), ws=None) == -22 and b"NULL" in err()
    chunk = [0x1000] * 6
    chunk[3] = 0x1004
    assert finish(L, stage_cfg(L), chunk=chunk) == -22 and b"16-byte" in err()
    # the packing entry
    pack = L.lib().cnerf_pack_pfilm_map_transposed
    assert pack(ctypes.byref(stage_cfg(L)), None, ctypes.c_void_p(0x1000), None) == -22 and b"NULL" in err()
    assert pack(ctypes.byref(stage_cfg(L)), ctypes.byref(L.FieldParams()), ctypes.c_void_p(0x1000), None) == -22 and b"NULL" in err()
    assert pack(ctypes.byref(stage_cfg(L, kinds=("sine",) * 3)), ctypes.byref(L.FieldParams()), ctypes.c_void_p(0x1000), None) == -22


def test_one_call_entries_size_the_fp32_backward_from_the_documented_pieces(L):
    """cnerf_render_backward / cnerf_field_query_backward run this family's exact backward themselves: their workspace is the pieces
    include/cnerf.h documents -- d rgb_sigma of both passes (render), the five chunk matrices of cnerf_field_backward, the chunk's sample
    positions (render), the stage's workspace and packed_map as cnerf_pfilm_finish_bytes reports them, a query's input-gradient rows
    (points_per_chunk, 256) -- each padded to 256 bytes at most, and nothing else."""
    lib, err = L.lib(), lambda: L.lib().cnerf_last_error()
    cfg = stage_cfg(L)
    cfg.R, cfg.S, cfg.fov_deg, cfg.flags = 8, 4, 30.0, L.F_HIERARCHICAL
    Lc, H, B, npi = 8, 256, 2, 8 * 8 * 4
    nbytes = ctypes.c_size_t()
    chunk_floats = lambda n: n * 32 + (Lc * n * H + n * 256) + 3 * Lc * n * H + 3 * Lc * n * H + n * 4
    for cnt in (1, 2):
        assert lib.cnerf_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_FP32, cnt, 0, ctypes.byref(nbytes)) == 0, err()
        rc, pm, fin = finish_bytes(L, cfg, cnt, npi)
        assert rc == 0
        n = cnt * npi
        raw = 2 * B * npi * 4 * 4 + chunk_floats(n) * 4 + n * 3 * 4 + fin + pm
        assert raw <= nbytes.value <= raw + 256 * 16, (cnt, raw, nbytes.value)
    for ppc in (1024, 4099):
        assert lib.cnerf_field_query_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_FP32, ppc, ctypes.byref(nbytes)) == 0, err()
        rc, pm, fin = finish_bytes(L, cfg, 1, ppc)
        assert rc == 0
        raw = chunk_floats(ppc) * 4 + fin + pm + ppc * 256 * 4
        assert raw <= nbytes.value <= raw + 256 * 16, (ppc, raw, nbytes.value)


def test_one_call_entries_refuse_what_the_fp32_backward_cannot_do(L):
    lib, err = L.lib(), lambda: L.lib().cnerf_last_error()
    n = ctypes.c_size_t()

    def render_cfg(precision):
        cfg = stage_cfg(L, precision=precision)
        cfg.R, cfg.S, cfg.fov_deg = 8, 4, 30.0
        return cfg

    # the fp32 chain re-runs the fp32 kernel, the fp16 chain the fp16x3 kernel; kept activations are the fp16 backward's
    for sizes, arg in ((lib.cnerf_backward_workspace_bytes, (1, 0)), (lib.cnerf_field_query_backward_workspace_bytes, (1024,))):
        assert sizes(ctypes.byref(render_cfg("fp16x3")), L.PREC_FP32, *arg, ctypes.byref(n)) == -22 and b"fp32" in err()
        assert sizes(ctypes.byref(render_cfg("fp32")), L.PREC_FP16, *arg, ctypes.byref(n)) == -22 and b"fp16x3" in err()
    assert lib.cnerf_backward_workspace_bytes(ctypes.byref(render_cfg("fp32")), L.PREC_FP32, 2, 1, ctypes.byref(n)) == -22 and b"kept activations" in err()
    # the call itself, made-up aligned addresses: a gradient struct without the mapping network's buffers is refused before any launch
    p, a = ctypes.c_void_p, 0x1000
    vols, gvols, fp, saved = L.Volumes(), L.Volumes(), L.FieldParams(), L.Saved()
    vols.level[0] = gvols.level[0] = a
    fp.map_w1 = fp.map_w2 = fp.w_final = a
    saved.coarse_rgb_sigma = saved.coarse_z = a
    g = L.FieldParamGrads()
    g.map_w1 = g.map_b1 = g.map_b2 = g.w_final = g.b_final = a          # map_w2 stays NULL
    for l in range(8):
        g.w[l] = g.b[l] = a
    rc = lib.cnerf_render_backward(ctypes.byref(render_cfg("fp32")), L.PREC_FP32, 1, ctypes.byref(vols), ctypes.byref(fp), p(a), p(a), None, None, p(a),
                                   None, ctypes.byref(saved), None, p(a), None, ctypes.byref(g), None, None, ctypes.byref(gvols), None, p(a), None)
    assert rc == -22 and b"mapping network" in err()
