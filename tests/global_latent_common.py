"""Shared by tests/test_global_latent_cpu.py and tests/test_gpu_global_latent.py: the aux_shortsiren_* / aux_pointnet_small fixtures
(tests/golden/make_golden_global.py) and a short float64-capable restatement of the global-latent network -- CustomMappingNetwork,
four FiLM layers on the world position, head with sigmoid on rgb (siren.py:55-78, 1172-1224 of the reference) -- composed with
the oracle's ray stages (oracle/render_oracle.py) into the whole render.  TEST INFRASTRUCTURE ONLY.

A fixture is several files, <name>.npz and <name>.part<i>.npz, each below 1 MiB (the wide Linears of the mapping MLP and their
gradients are stored in full and do not compress); Fixture reads them as one."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR
from oracle import render_oracle as O

N_LAYERS = 4


class Fixture:
    """All parts of one fixture: arrays by key, `meta` from the JSON string."""

    def __init__(self, name):
        self.name = name
        self.arrays = {}
        parts = sorted(f for f in os.listdir(GOLDEN_DIR) if f == name + ".npz" or (f.startswith(name + ".part") and f.endswith(".npz")))
        assert parts and parts[0] == name + ".npz", name
        for f in parts:
            with np.load(os.path.join(GOLDEN_DIR, f)) as d:
                for k in d.files:
                    assert k not in self.arrays, k
                    self.arrays[k] = d[k]
        self.files = list(self.arrays)
        self.meta = json.loads(bytes(self.arrays["meta_json"]).decode())

    def __contains__(self, k):
        return k in self.arrays

    def __getitem__(self, k):
        return self.arrays[k]

    def get(self, k):
        return self.arrays.get(k)


def fixture(name):
    return Fixture(name)


def stored_params(g, prefix=""):
    """state dict stored in the fixture under param/<prefix>"""
    p = "param/" + prefix
    return {k[len(p):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p)}


def make_generator(g, drop_out=0):
    """ImplicitGenerator3d("SHORTSIREN") with the fixture's stored parameters (the reference's, head scaled), strict."""
    from cnerf_amd.generators import ImplicitGenerator3d
    m = g.meta
    torch.manual_seed(m["seed"])
    gen = ImplicitGenerator3d("SHORTSIREN", z_dim=m["Z"], input_dim=3, output_dim=4, hidden_dim=m["H"], drop_out=drop_out)
    gen.load_state_dict(stored_params(g), strict=True)
    return gen


def fresh_generator(H, Z=32, seed=0, drop_out=0, sigma_scale=20.0):
    from cnerf_amd.generators import ImplicitGenerator3d
    torch.manual_seed(seed)
    gen = ImplicitGenerator3d("SHORTSIREN", z_dim=Z, input_dim=3, output_dim=4, hidden_dim=H, drop_out=drop_out)
    with torch.no_grad():
        gen.siren.final_layer.weight[3] *= sigma_scale
    return gen


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: params = state dict of generator.siren (any dtype), differentiable
# ---------------------------------------------------------------------------------------------------------------------
def mapping(params, z):
    """CustomMappingNetwork: Linear, LeakyReLU(0.2) three times, Linear -> (frequencies, phase_shifts)."""
    x = z
    for i in (0, 2, 4):
        x = F.leaky_relu(F.linear(x, params[f"mapping_network.network.{i}.weight"], params[f"mapping_network.network.{i}.bias"]), 0.2)
    fo = F.linear(x, params["mapping_network.network.6.weight"], params["mapping_network.network.6.bias"])
    half = fo.shape[-1] // 2
    return fo[..., :half], fo[..., half:]


def field(params, z, points, drop=None):
    """rgb_sigma (B,N,4) at points (B,N,3).  drop = (p, keep (n_layers, B, N, H)): training mode with these keep decisions."""
    H = params["final_layer.weight"].shape[1]
    freq, phase = mapping(params, z)
    freq = freq * 15 + 30
    x = points
    for i in range(N_LAYERS):
        pre = F.linear(x, params[f"network.{i}.layer.weight"], params[f"network.{i}.layer.bias"])
        x = torch.sin(freq[:, None, i * H:(i + 1) * H] * pre + phase[:, None, i * H:(i + 1) * H])
        if drop is not None:
            x = x * drop[1][i].to(x.dtype) * (1.0 / (1.0 - drop[0]))
    out = F.linear(x, params["final_layer.weight"], params["final_layer.bias"])
    return torch.cat([torch.sigmoid(out[..., :3]), out[..., 3:]], -1)


def render(params, z, cam2world, meta, u_strat, u_fine, eps_coarse=None, eps_final=None, forced_fine_z=None, drop=None, R=None, S=None):
    """The whole render, like oracle.render_oracle.render with this field: rays, depths and positions in fp32 under no_grad (they
    carry no gradient), the field in the dtype of params / z.  drop = (p, keep_coarse, keep_fine).  -> (pixels, depth, aux)"""
    R, S = R or meta["R"], S or meta["S"]
    B, P = cam2world.shape[0], R * R
    dt = z.dtype
    with torch.no_grad():
        dirs_cam = O.camera_ray_dirs(R, meta["fov"])
        z_lin, offset, zc = O.stratified_depths(B, R, S, meta["ray_start"], meta["ray_end"], u_strat)
        pts, dirs_w, origins = O.coarse_world_points(cam2world, dirs_cam, z_lin, offset)
    c_out = field(params, z, pts.reshape(B, P * S, 3).to(dt), None if drop is None else (drop[0], drop[1])).reshape(B, P, S, 4)
    noise, clamp = meta["noise"], meta["clamp"]
    with torch.no_grad():
        _, _, w = O.composite(c_out.float(), zc, eps_coarse, noise, clamp)
        fine_z, inds, cdf = O.importance_depths(zc, w, u_fine)
        resampled = fine_z
        if forced_fine_z is not None:
            fine_z = forced_fine_z.reshape(B, P, S)
        fpts = origins.reshape(B, 1, 1, 3) + dirs_w.unsqueeze(2) * fine_z.unsqueeze(-1)
    f_out = field(params, z, fpts.reshape(B, P * S, 3).to(dt), None if drop is None else (drop[0], drop[2])).reshape(B, P, S, 4)
    all_out, all_z, sort_idx = O.merge_by_depth(f_out, c_out, fine_z.to(dt), zc.to(dt))
    rgb, dist, wfin = O.composite(all_out, all_z, None if eps_final is None else eps_final.to(dt), noise, clamp, meta["white_back"], meta["last_back"])
    pixels = rgb.reshape(B, R, R, 3).permute(0, 3, 1, 2).contiguous() * 2 - 1
    depth = (dirs_cam[:, 2].reshape(1, P).to(dt) * dist).reshape(B, R, R)
    aux = dict(coarse_points=pts, coarse_z=zc, coarse_rgb_sigma=c_out, coarse_weights=w, cdf=cdf, inds=inds, resampled_z=resampled, fine_z=fine_z,
               fine_points=fpts, fine_rgb_sigma=f_out, sort_idx=sort_idx, final_weights=wfin)
    return pixels, depth, aux


def cast_params(net, dtype, requires_grad=False):
    return {k: v.detach().clone().to(dtype).requires_grad_(requires_grad) for k, v in net.state_dict().items()}
