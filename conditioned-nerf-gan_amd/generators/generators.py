"""ImplicitGenerator3d: the generator API of the reference (generators/generators.py:9-197), backed by the gfx950
render path.  Same constructor, attributes, forward signature and state-dict keys, so the reference's
train.py / inference.py / extract_shapes.py call sites work unchanged:

    pixels, depth_map = generator(z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps,
                                  hierarchical_sample, **metadata)
"""
import torch
import torch.nn as nn

from . import siren
from .. import ops

OccupancyGrid = ops.OccupancyGrid      # what build_occupancy returns


def draw_rng(B, P, S, hierarchical, noise_std, dev):
    """The random tensors of one forward, drawn with the reference's shapes and in its order (rand (B,P,S,1),
    randn (B,P,S,1), rand (B*P,S), randn (B,P,2S,1)), so the torch generator advances exactly as it does there; the noise
    tensors are drawn even when nerf_noise == 0 (volumetric_rendering.py:39) and only handed on when they are used."""
    rng = {"u_strat": torch.rand((B, P, S, 1), device=dev)}
    if hierarchical:
        eps_c = torch.randn((B, P, S, 1), device=dev)
        rng["u_fine"] = torch.rand((B * P, S), device=dev)
        eps_f = torch.randn((B, P, 2 * S, 1), device=dev)
        if noise_std != 0:
            rng["eps_coarse"], rng["eps_final"] = eps_c, eps_f
    else:
        eps_f = torch.randn((B, P, S, 1), device=dev)
        if noise_std != 0:
            rng["eps_final"] = eps_f
    return rng


class ImplicitGenerator3d(nn.Module):
    _instances = 0

    def _philox_key(self):
        """(seed, offset) of this forward's in-kernel draws: see __init__."""
        if self._rng_step != self.step:
            self._rng_step, self._rng_calls = self.step, 0
        offset = ((int(self.step) & 0xFFFFFF) << 8) | (self._rng_calls & 0xFF)
        self._rng_calls += 1
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        seed = (torch.cuda.initial_seed() + 0x9E3779B97F4A7C15 * (self._rng_salt + 1) + 0xD1B54A32D192ED03 * rank) & 0xFFFFFFFFFFFFFFFF
        return seed, offset

    def __init__(self, siren_type, z_dim, input_dim, output_dim, hidden_dim, drop_out=0):
        super().__init__()
        self.z_dim = z_dim
        field_cls = getattr(siren, siren_type)
        self.siren = field_cls(z_dim=z_dim, input_dim=input_dim, output_dim=output_dim, hidden_dim=hidden_dim,
                               drop_out=drop_out, device=None)
        self.epoch = 0
        self.step = 0
        self.device = None
        # where the four random draws of a forward come from: "torch" (torch.rand / randn on the device in the reference's
        # order and shapes -- the default: the torch generator advances as it does there) or "philox" (in-kernel)
        self.rng_mode = "torch"
        # Key and counter of the in-kernel draws (rng_mode "philox", dropout decisions).  Key = torch's CUDA seed mixed with a salt that
        # is different for every generator of the process (a teacher and a student under one seed must not draw the same streams) and
        # with the rank of a distributed job (ranks seeded alike still draw their own).  Counter offset = (self.step, calls within
        # that step): `step` is what checkpoints store (utils.py:467), so a resumed run continues the stream instead of replaying the
        # draws of steps 0..k -- nothing else has to be persisted.
        self._rng_salt = ImplicitGenerator3d._instances
        ImplicitGenerator3d._instances += 1
        self._rng_step, self._rng_calls = None, 0

    def set_device(self, device):
        self.device = device
        self.siren.device = device

    def forward(self, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, hierarchical_sample, **kwargs):
        """z: feature volume (B,C,V,V,V) or (feature volume, global feature (B,z_dim)); SHORTSIREN: the latent (B,z_dim) alone.
        kwargs read: clamp_mode, nerf_noise (required, like the reference), white_back, last_back; every other key
        of the splatted metadata dict is ignored.  `_rng` (dict of tensors) injects the four random draws and
        `_aux` (dict) receives intermediates, `_field_events` (4 hipEvent_t handles) times the field kernel -- test and
        benchmark hooks the reference does not have.
        Returns pixels (B,3,R,R) = 2*rgb-1 and depth_map (B,R,R)."""
        net = self.siren
        net.check_supported()
        clamp_mode, noise_std = kwargs["clamp_mode"], kwargs["nerf_noise"]
        white_back, last_back = kwargs.get("white_back", False), kwargs.get("last_back", False)
        fvol, glob = net.split_z(z)
        B, R, S = cam2worlds.shape[0], int(img_size), int(num_steps)
        dev = cam2worlds.device
        freq, phase = net.film(glob)
        rng = kwargs.get("_rng")
        if rng is None:
            if self.rng_mode == "philox":
                # draws generated inside the kernels (Philox4x32-10): no RNG kernels, no tensors; keyed per module, one counter value
                # per forward (see __init__)
                rng = {"philox": self._philox_key()}
            else:
                rng = draw_rng(B, R * R, S, bool(hierarchical_sample), noise_std, dev)
        if net.drop_out and net.training and "drop" not in rng:
            # dropout decisions are Philox draws inside the field kernels (or rng["drop_coarse"/"drop_fine"] bytes), keyed like
            # the philox rng mode
            rng = dict(rng, drop=(float(net.drop_out), rng.get("philox") or self._philox_key()))
        aux_out = kwargs.get("_aux")
        pixels, depth, aux = ops.render(net, fvol, freq, phase, cam2worlds, R, fov, ray_start, ray_end, S,
                                        bool(hierarchical_sample), clamp_mode, noise_std, white_back, last_back, rng,
                                        want_aux=aux_out is not None, field_events=kwargs.get("_field_events"))
        if aux_out is not None:
            aux_out.update(aux)
        return pixels, depth

    def render_rays(self, z, origins, dirs, ray_start, ray_end, num_steps, hierarchical_sample, **kwargs):
        """`forward` on rays the caller formed instead of the square pinhole grid: a crop or a non-square image, a random subset of
        pixels, intrinsics with a principal-point offset, one tile of a large image (volumetric_rendering.pinhole_rays makes the
        grid's rays for any rows / columns).  origins, dirs: (B,P,3) world; directions are not normalised here and depths are in
        units of |dir|.  z and the kwargs as in `forward`: clamp_mode and nerf_noise are required; white_back, last_back, `_rng` and
        `_aux` optional.  rng_mode "torch" draws as `forward` does for P rays (draw_rng(B, P, S, ...): same order and shapes),
        "philox" draws in the kernels.  Differentiable w.r.t. everything `forward` is, and w.r.t. origins and dirs (the sample
        depths carry no gradient, as in the reference).  Dropout is not implemented here: a training-mode network with
        drop_out > 0 raises NotImplementedError.
        occupancy=grid (an OccupancyGrid of build_occupancy, one grid per image): samples in cells whose bit is clear are not given to
        the field network -- forward only: raises when grad mode is on and any of z, the parameters, origins or dirs requires grad, and
        when the grid's batch is not B; `_aux` then also receives live_coarse / live_fine, (B,) int32: the points each pass evaluated.
        Without the key the call is what it was.
        ray_near=near, ray_far=far (both (B,P), e.g. from ray_bounds; both or neither): the coarse samples of ray (b,p) are stratified
        over [near, far] instead of [ray_start, ray_end]; the fine pass resamples inside that span as it always did.  With and without
        `occupancy`, and differentiable like the unbounded call: the bounds themselves are detached and get no gradient.  ValueError:
        only one of the two, or a shape other than (B,P).  Without the keys the call is what it was.
        Returns pixels (B,P,3) = 2*rgb-1 and dist (B,P) = sum of weight * depth along the ray."""
        net = self.siren
        net.check_supported()
        if net.drop_out and net.training:
            raise NotImplementedError("render_rays has no dropout: call eval() first, or use forward, the path that has dropout")
        near, far = kwargs.get("ray_near"), kwargs.get("ray_far")
        if (near is None) != (far is None):
            raise ValueError("render_rays: ray_near and ray_far must both be given, or neither")
        if near is not None and (tuple(near.shape) != tuple(origins.shape[:2]) or tuple(far.shape) != tuple(origins.shape[:2])):
            raise ValueError(f"render_rays: ray_near and ray_far must be (B,P) = {tuple(origins.shape[:2])}, got {tuple(near.shape)} and {tuple(far.shape)}")
        occupancy = kwargs.get("occupancy")
        if occupancy is not None:
            fv, gl = net.split_z(z)
            zs = [t for t in (*ops.as_levels(fv), gl) if torch.is_tensor(t)]
            if torch.is_grad_enabled() and any(t.requires_grad for t in (*zs, *self.parameters(), origins, dirs)):
                raise RuntimeError("render_rays(occupancy=...) is forward only: call it under torch.no_grad()")
            if occupancy.bits.shape[0] != origins.shape[0]:
                raise ValueError(f"occupancy holds {occupancy.bits.shape[0]} grids, the call renders {origins.shape[0]} images")
        clamp_mode, noise_std = kwargs["clamp_mode"], kwargs["nerf_noise"]
        white_back, last_back = kwargs.get("white_back", False), kwargs.get("last_back", False)
        fvol, glob = net.split_z(z)
        B, P, S = origins.shape[0], origins.shape[1], int(num_steps)
        freq, phase = net.film(glob)
        rng = kwargs.get("_rng")
        if rng is None:
            rng = {"philox": self._philox_key()} if self.rng_mode == "philox" else draw_rng(B, P, S, bool(hierarchical_sample), noise_std, origins.device)
        aux_out = kwargs.get("_aux")
        pixels, dist, aux = ops.render_rays(net, fvol, freq, phase, origins, dirs, ray_start, ray_end, S, bool(hierarchical_sample), clamp_mode,
                                            noise_std, white_back, last_back, rng, want_aux=aux_out is not None,
                                            **({} if occupancy is None else {"occupancy": occupancy}),
                                            **({} if near is None else {"near": near, "far": far}))
        if aux_out is not None:
            aux_out.update(aux)
        return pixels, dist

    def ray_bounds(self, grid, origins, dirs, ray_start, ray_end, pad=None):
        """Per-ray sampling bounds for render_rays(..., ray_near=near, ray_far=far) from an OccupancyGrid of build_occupancy: the span of
        [ray_start, ray_end] over which ray (b,p) crosses set cells of image b's grid, widened by `pad` on both sides and clamped to
        [ray_start, ray_end].  A ray that crosses no set cell has hit = 0 and keeps [ray_start, ray_end].  Outside the grid's cube a ray
        counts as empty (unlike the masked render, which skips nothing there): choose a cube that covers the density.
        pad is a depth, in units of |dir| like ray_start / ray_end; None: half a cell edge, 0.5 * side / G, which is a length in space --
        right for unit directions; for unnormalised rays pass pad = 0.5 * side / G / |dir| yourself (one number, e.g. for the shortest
        direction).  Choose pad no smaller than half a coarse step, (far - near) / (2 (num_steps - 1)): the jitter moves the last
        coarse sample that far to either side of `far`, the compositing gives a ray's last sample an unbounded interval (as the
        reference does), and a last sample inside density is opaque (profiles/ray_bounds.md: the default loses at 16 samples).
        No gradient flows through the bounds.
        Returns near, far (B,P) float32 and hit (B,P) uint8."""
        if pad is None:
            pad = 0.5 * float(grid.side) / int(grid.G)
        if grid.bits.shape[0] != origins.shape[0]:
            raise ValueError(f"occupancy holds {grid.bits.shape[0]} grids, the call has rays of {origins.shape[0]} images")
        with torch.no_grad():
            return ops.occupancy_ray_bounds(grid, origins, dirs, ray_start, ray_end, pad)

    def build_occupancy(self, z, lo, side, resolution=64, threshold=0.0, dilate=1, max_points=1 << 22):
        """Occupancy grids of the scenes z for render_rays(..., occupancy=grid): build once, render many cameras.  The density is queried
        at the (G+1)^3 corners lo + i (side / G), G = resolution (a multiple of 4 in [4,256]), of the cube with corner lo (3 floats) and
        edge side -- self.siren(points, z) under no_grad, max_points per image at a time -- and cnerf_occupancy_build sets the bit of every
        cell whose corners, or those of a cell within `dilate` of it, exceed `threshold` (include/cnerf.h has the exact rule).  Density
        between the corners is not seen: choose the resolution for the field's detail, and dilate.
        Returns OccupancyGrid(bits (B, G^3 / 32) int32, lo, side, G)."""
        net = self.siren
        G = int(resolution)
        if G % 4 or not 4 <= G <= 256:
            raise ValueError(f"resolution={G} must be a multiple of 4 in [4,256]")
        lo = tuple(float(v) for v in lo)
        with torch.no_grad():
            fvol, glob = net.split_z(z)
            ref = glob if glob is not None else ops.as_levels(fvol)[0]
            B, dev = ref.shape[0], ref.device
            i = torch.arange(G + 1, device=dev, dtype=torch.float32)
            step = torch.tensor(float(side), device=dev, dtype=torch.float32) / G
            ax = [torch.tensor(v, device=dev, dtype=torch.float32) + i * step for v in lo]
            pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(1, -1, 3)
            chunk = max(1, int(max_points))
            sigma = torch.cat([net(pts[:, p0:p0 + chunk].expand(B, -1, -1).contiguous(), z)[..., 3] for p0 in range(0, pts.shape[1], chunk)], 1)
            bits = ops.occupancy_build(sigma, G, threshold, dilate)
        return ops.OccupancyGrid(bits, lo, float(side), G)

    def generate_avg_frequencies(self):
        """Mean FiLM frequencies / phase shifts over 10000 random latents (generators.py:189-197)."""
        zs = torch.randn((10000, self.z_dim), device=self.siren.device)
        with torch.no_grad():
            fo = self.siren.mapping_network(zs)
        if isinstance(fo, tuple):       # a mapping MLP returns (frequencies, phase_shifts) itself
            fr, ph = fo
        else:
            half = fo.shape[-1] // 2
            fr, ph = fo[..., :half], fo[..., half:]
        self.avg_frequencies = fr.mean(0, keepdim=True)
        self.avg_phase_shifts = ph.mean(0, keepdim=True)
        return self.avg_frequencies, self.avg_phase_shifts
