"""Host code of the field-query backward (ABI v9), no GPU: workspace sizing and what the call refuses."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def query_cfg(L, kinds=("film",) * 4, precision="fp32", B=3, H=128):
    cfg = L.Cfg()
    cfg.B, cfg.V, cfg.C, cfg.H, cfg.L = B, 16, 32, H, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = L.LAYER_CODE[k]
    cfg.voxel_length = 1.2
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, 16, 32
    cfg.precision = L.PREC_CODE[precision]
    return cfg                      # R, S, fov left at 0: a query does not read them


def ws_bytes(L, cfg, bprec, ppc):
    n = ctypes.c_size_t()
    rc = L.lib().cnerf_field_query_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_CODE[bprec], ppc, ctypes.byref(n))
    return rc, n.value


def test_query_workspace_grows_with_the_chunk_not_with_the_call(L):
    for precision, bprec in (("fp32", "fp32"), ("fp16x3", "fp16")):
        cfg = query_cfg(L, precision=precision)
        sizes = []
        for ppc in (1000, 4096, 1 << 20):
            rc, nb = ws_bytes(L, cfg, bprec, ppc)
            assert rc == 0, L.lib().cnerf_last_error()
            sizes.append(nb)
        assert sizes[0] < sizes[1] < sizes[2]
        assert sizes[2] >= (1 << 20) * 3 * 4 * 128 // (2 if bprec == "fp16" else 1)     # the gradient slabs of 4 matrices, at least
        cfg.B = 64                                     # the call's image count does not enter the chunk buffers
        assert ws_bytes(L, cfg, bprec, 4096) == (0, sizes[1])
    # TALLSIREN's fp16 chain
    cfg = query_cfg(L, kinds=("pfilm",) * 8, precision="fp16x3")
    a, b = ws_bytes(L, cfg, "fp16", 1000), ws_bytes(L, cfg, "fp16", 2000)
    assert a[0] == 0 and b[0] == 0 and b[1] > a[1]


def test_query_backward_refusals(L):
    assert ws_bytes(L, query_cfg(L, precision="fp32"), "fp16", 1024)[0] == -22          # the fp16 backward re-runs the fp16x3 forward
    assert b"fp16x3" in L.lib().cnerf_last_error()
    # per-point FiLM, exact fp32: runs here on an fp32 cfg -- the chunk matrices (3 L gradient slabs alone), and grows with the chunk
    rc, pw = ws_bytes(L, query_cfg(L, kinds=("pfilm",) * 8, precision="fp32"), "fp32", 1024)
    assert rc == 0 and pw >= 1024 * 3 * 8 * 128 * 4 and ws_bytes(L, query_cfg(L, kinds=("pfilm",) * 8, precision="fp32"), "fp32", 2048)[1] > pw
    assert ws_bytes(L, query_cfg(L, kinds=("pfilm",) * 8, precision="fp16x3"), "fp32", 1024)[0] == -22 and b"fp32" in L.lib().cnerf_last_error()
    assert ws_bytes(L, query_cfg(L), "fp32", 0)[0] == -22
    cfg = query_cfg(L)
    cfg.drop_p = 0.2
    rc, with_drop = ws_bytes(L, cfg, "fp32", 1024)
    assert rc == 0 and with_drop > ws_bytes(L, query_cfg(L), "fp32", 1024)[1]       # the chunk's keep bytes
    # no launch is attempted on bad arguments
    assert L.lib().cnerf_field_query_backward(ctypes.byref(query_cfg(L)), 0, 1024, None, None, None, None, None, None, None, 10, None, None,
                                              None, None, None, None, None, None, None, None) == -22
