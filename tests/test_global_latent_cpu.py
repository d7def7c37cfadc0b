"""CPU checks of the global-latent setting (SHORTSIREN: FiLM field on world positions, no feature volume; PointNet encoder): module
and init parity with the reference (fixtures of tests/golden/make_golden_global.py), host validation of CNERF_F_NO_VOLUME, the
point-cloud path of the GAN step with a stand-in generator.  No GPU compute."""
import ctypes

import numpy as np
import pytest
import torch

import global_latent_common as G


def test_shortsiren_init_and_state_dict_match_reference():
    """Same torch seed -> the reference's state-dict keys and every parameter bit for bit, the four mapping Linears and the head as
    the constructor drew it included; the restatement agrees with the reference's own rgb_sigma at the reference's own points."""
    from cnerf_amd.generators import ImplicitGenerator3d, siren
    g = G.fixture("aux_shortsiren_small")
    m = g.meta
    torch.manual_seed(m["seed"])
    gen = ImplicitGenerator3d("SHORTSIREN", z_dim=m["Z"], input_dim=3, output_dim=4, hidden_dim=m["H"])
    sd = gen.state_dict()
    ref = G.stored_params(g)
    assert set(sd) == set(ref)
    assert {"siren.network.3.layer.weight", "siren.final_layer.bias", "siren.mapping_network.network.6.weight"} <= set(sd)
    assert all(f"siren.mapping_network.network.{i}.bias" in sd for i in (0, 2, 4, 6))
    for k, v in sd.items():
        want = g["init/" + k] if "final_layer" in k else ref[k].numpy()      # (the fixture's head is scaled after construction)
        assert v.shape == want.shape and np.array_equal(v.numpy(), want), k
    gen.load_state_dict(ref, strict=True)
    assert isinstance(gen.siren.mapping_network, siren.CustomMappingNetwork)
    assert gen.step == 0 and gen.epoch == 0
    # the restatement used by the GPU tests reproduces the reference's own outputs (fp32, same operations)
    gen = G.make_generator(g)
    params = {k: v for k, v in gen.siren.state_dict().items()}
    z = torch.from_numpy(g["z"])
    B = z.shape[0]
    with torch.no_grad():
        out = G.field(params, z, torch.from_numpy(g["coarse_points"]).reshape(B, -1, 3))
    assert np.abs(out.numpy().reshape(g["coarse_rgb_sigma"].shape) - g["coarse_rgb_sigma"]).max() < 2e-5
    with pytest.raises(NotImplementedError):
        ImplicitGenerator3d("SHORTSIREN", z_dim=8, input_dim=2, output_dim=4, hidden_dim=64).siren.check_supported()
    gen.generate_avg_frequencies()
    assert gen.avg_frequencies.shape == (1, 4 * m["H"]) and gen.avg_phase_shifts.shape == (1, 4 * m["H"])


def test_mapping_network_and_pointnet_match_reference():
    """CustomMappingNetwork and ResnetPointnet against the reference's stored outputs (tolerance of the U-Net fixture in
    test_training_cpu.py: 1e-5 absolute); encode_pcl with noise_weight 0 reproduces z and l_reg."""
    from cnerf_amd.generators.siren import CustomMappingNetwork
    from cnerf_amd.training.encoder import ResnetPointnet, encode_pcl
    g = G.fixture("aux_pointnet_small")
    m = g.meta
    torch.manual_seed(m["seed"])
    mp = CustomMappingNetwork(m["c_dim"], m["map_hidden"], m["map_out"])
    assert set(mp.state_dict()) == {f"network.{i}.{p}" for i in (0, 2, 4, 6) for p in ("weight", "bias")}
    ref = G.stored_params(g, "map/")
    assert set(ref) == set(mp.state_dict())
    for k, v in mp.state_dict().items():
        assert np.array_equal(v.numpy(), ref[k].numpy()), k
    enc = ResnetPointnet(c_dim=m["c_dim"], dim=m["dim"], hidden_dim=m["hidden_dim"])
    enc.load_state_dict(G.stored_params(g, "enc/"), strict=True)
    enc.eval()
    pcl = torch.from_numpy(g["pcl"])
    with torch.no_grad():
        codes = enc(pcl)
        z, l_reg = encode_pcl(enc, pcl, torch.device("cpu"), noise_weight=0)
        freq, phase = mp(torch.from_numpy(g["z"]))
    assert np.abs(codes.numpy() - g["codes"]).max() < 1e-5
    assert np.abs(z.numpy() - g["z"]).max() < 1e-5
    assert abs(float(l_reg) - float(g["l_reg"])) < 1e-5
    assert np.abs(freq.numpy() - g["frequencies"]).max() < 1e-5 and np.abs(phase.numpy() - g["phase_shifts"]).max() < 1e-5
    # l_reg is taken before the normalisation; the rows of z are normalised
    assert abs(float(l_reg) - float(codes.norm(dim=1).mean())) < 1e-6
    assert z.mean(1).abs().max() < 1e-5 and (z.std(1) - 1).abs().max() < 1e-5


def _cfg(L, flags, C=0, H=64, kinds=(0, 0, 0, 0), precision=0):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = 2, 6, 10, 0, C, H, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.voxel_length, cfg.fov_deg, cfg.flags, cfg.precision = 1.2, 30.0, flags, precision
    return cfg


def test_no_volume_host_validation():
    """CNERF_F_NO_VOLUME on the host side, without a GPU: the size queries accept C = 0, fvol_cl is 0, the excluded combinations
    are refused with -22, and so is C = 0 without the flag."""
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    assert L.ABI_VERSION == 10 and lib.cnerf_abi_version() == 10
    NV = L.F_NO_VOLUME | L.F_SIGMOID_RGB | L.F_HIERARCHICAL
    a, b, c, n = (ctypes.c_size_t(7) for _ in range(4))
    cfg = _cfg(L, NV)
    assert lib.cnerf_workspace_bytes(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib.cnerf_last_error()
    assert b.value == 0 and a.value > 0 and c.value >= 2 * 360 * 10 * 4
    # packed: layer 0 is one k-tile (K = 3 padded), not C / 32 of them
    assert a.value < (2 * 64 * 32 + 3 * 64 * 64 + 32 * 64 + 6 * 64 + 4) * 4 + 256
    assert lib.cnerf_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_FP32, 2, 0, ctypes.byref(n)) == 0, lib.cnerf_last_error()
    assert n.value > 0
    assert lib.cnerf_field_query_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_FP32, 4099, ctypes.byref(n)) == 0, lib.cnerf_last_error()
    assert lib.cnerf_backward_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value > 0
    # residual and plain-sine layers are allowed
    assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, NV, kinds=(1, 2, 0))), ctypes.byref(a), None, None) == 0
    # refusals
    assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, NV, kinds=(3, 3))), ctypes.byref(a), None, None) == -22
    assert b"per-point FiLM" in lib.cnerf_last_error()
    assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, NV | L.F_INPUT_XYZ)), ctypes.byref(a), None, None) == -22
    assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, NV, C=32)), ctypes.byref(a), None, None) == -22
    assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, L.F_SIGMOID_RGB)), ctypes.byref(a), None, None) == -22
    assert b"C=0" in lib.cnerf_last_error()
    # the lookup / scatter entry points refuse the flag with a message (no launch is attempted)
    one = ctypes.c_void_p(256)
    assert lib.cnerf_gather_features(ctypes.byref(cfg), one, one, 1, one, None) == -22 and b"NO_VOLUME" in lib.cnerf_last_error()
    assert lib.cnerf_scatter_features(ctypes.byref(cfg), one, 1, one, one, None) == -22 and b"NO_VOLUME" in lib.cnerf_last_error()
    vs = L.Volumes()
    assert lib.cnerf_feature_points_grad(ctypes.byref(cfg), ctypes.byref(vs), one, 1, one, one, None) == -22 and b"NO_VOLUME" in lib.cnerf_last_error()
    # the fp16 arithmetics: sizes of both forward layouts, the half-precision chain's packing and workspaces (which reserve no
    # input-gradient rows for the patch scatter: there is no feature tile)
    for prec in (L.PREC_FP16X3, L.PREC_FP16):
        assert lib.cnerf_workspace_bytes(ctypes.byref(_cfg(L, NV, precision=prec)), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib.cnerf_last_error()
        assert b.value == 0
    c16 = _cfg(L, NV, precision=L.PREC_FP16X3)
    with_rows = _cfg(L, L.F_SIGMOID_RGB | L.F_HIERARCHICAL, C=32, precision=L.PREC_FP16X3)
    with_rows.V = 8
    n_fg = ctypes.c_size_t()
    assert lib.cnerf_backward_workspace_bytes(ctypes.byref(c16), L.PREC_FP16, 2, 0, ctypes.byref(n)) == 0, lib.cnerf_last_error()
    assert lib.cnerf_backward_workspace_bytes(ctypes.byref(with_rows), L.PREC_FP16, 2, 0, ctypes.byref(n_fg)) == 0, lib.cnerf_last_error()
    assert n_fg.value - n.value >= 2 * 360 * 32 * 4          # SHORTSIREN_FG's rows of the same shape: (1 tile, 720 points, 32) fp32
    assert lib.cnerf_field_query_backward_workspace_bytes(ctypes.byref(c16), L.PREC_FP16, 4099, ctypes.byref(n)) == 0, lib.cnerf_last_error()
    assert lib.cnerf_backward16_bytes(ctypes.byref(c16), ctypes.byref(n)) == 0 and n.value > 0
    # dropout stays fp32-only
    drop = _cfg(L, NV, precision=L.PREC_FP16X3)
    drop.drop_p = 0.25
    assert lib.cnerf_workspace_bytes(ctypes.byref(drop), ctypes.byref(a), None, None) == -22


class _StandInGenerator(torch.nn.Module):
    """latent (B, z_dim), cameras, img_size, ... -> (pixels (B,3,R,R), depth (B,R,R)), differentiable w.r.t. its parameters and z."""

    def __init__(self, z_dim):
        super().__init__()
        self.lin = torch.nn.Linear(z_dim, 3 * 4 * 4)
        self.step = 0
        self.epoch = 0

    def forward(self, z, cam2worlds, img_size, *args, **kwargs):
        assert torch.is_tensor(z) and z.dim() == 2
        px = torch.tanh(self.lin(z)).reshape(-1, 3, 4, 4) + 0.01 * cam2worlds[:, :3, 3].reshape(-1, 3, 1, 1)
        px = torch.nn.functional.interpolate(px, size=(img_size, img_size), mode="bilinear", align_corners=False)
        return px, px.mean(1)


def test_gan_step_with_point_clouds():
    """default_metadata("SHORTSIREN") is the reference's generator dictionary with a PointNet encoder entry; GanTrainer with
    dataset.load_pcl encodes sample["pcl"], runs one D and one G step, and the G step's loss carries z_reg_weight * l_reg: with
    weight 1 the encoder's gradient differs from weight 0 by exactly d l_reg."""
    from cnerf_amd.training import GanTrainer, default_metadata
    from cnerf_amd.training.encoder import ResnetPointnet
    from cnerf_amd.training.gan_step import synthetic_sample
    md0 = default_metadata(img_size=16, num_steps=8, batch_size=2, batch_split=1, siren_type="SHORTSIREN", hidden_dim=64)
    assert md0["generator"] == {"siren_type": "SHORTSIREN", "z_dim": 512, "input_dim": 3, "output_dim": 4, "hidden_dim": 64}
    assert md0["dataset"]["load_pcl"] and not md0["dataset"]["load_voxel"] and md0["pointnet"]["dim"] == 6 and md0["pointnet"]["c_dim"] == 512
    assert "dataset" not in default_metadata(siren_type="SHORTSIREN_FG")        # the voxel setting is as it was
    runs = {}
    for weight in (0.0, 1.0):
        torch.manual_seed(3)
        np.random.seed(3)
        md = default_metadata(img_size=16, num_steps=8, batch_size=2, batch_split=1, siren_type="SHORTSIREN", hidden_dim=64)
        md["pointnet"] = {"c_dim": 16, "dim": 6, "hidden_dim": 16}
        md["z_reg_weight"] = weight
        md["grad_clip"] = 1e9                     # no clipping: the two runs' gradients are compared
        tr = GanTrainer(md, torch.device("cpu"), modules={"generator": _StandInGenerator(16)})
        assert isinstance(tr.encoder, ResnetPointnet)
        with torch.no_grad():                     # fc_1 starts at zero: give the residual branches weight
            for i in range(5):
                getattr(tr.encoder, f"block_{i}").fc_1.weight.normal_(0.0, 0.2, generator=torch.Generator().manual_seed(i))
        sample = synthetic_sample(2, 16, 8, "cpu", torch.Generator().manual_seed(9), pcl_points=64)
        assert sample["pcl"].shape == (2, 64, 6) and "voxel" not in sample
        before = [p.detach().clone() for p in tr.encoder.parameters()]
        seen = {}
        step = tr.optimizer_E.step
        tr.optimizer_E.step = lambda: (seen.update(grad=[p.grad.detach().clone() for p in tr.encoder.parameters()]), step())[1]
        tr.step(sample)
        assert np.isfinite(tr.losses["d"][-1]) and np.isfinite(tr.losses["g"][-1]) and np.isfinite(tr.losses["photo"][-1])
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, tr.encoder.parameters()))
        assert tr.last["z_reg"] > 0 and abs(tr.last["z_reg_loss"] - weight * tr.last["z_reg"]) < 1e-12
        # d l_reg / d encoder on the same clouds, by autograd
        enc = ResnetPointnet(**md["pointnet"])
        enc.load_state_dict({k: v for k, v in zip(tr.encoder.state_dict().keys(), before)})
        l_reg = enc(sample["pcl"]).norm(dim=1).mean()
        runs[weight] = (seen["grad"], torch.autograd.grad(l_reg, list(enc.parameters())), float(l_reg.detach()), tr.last["z_reg"])
    (g0, dreg, l_reg, seen_reg), (g1, _, _, _) = runs[0.0], runs[1.0]
    assert abs(l_reg - seen_reg) < 1e-5
    for a, b, d in zip(g0, g1, dreg):
        assert torch.allclose(b - a, d, rtol=1e-4, atol=1e-6)
