"""Shape metrics of a reconstruction: Chamfer distance and F-score between two batched point clouds, area-weighted samples of a triangle
mesh, and the end-to-end score of a conditioned scene against the cloud it was conditioned on (the reference reaches for the external
`chamferdist` CUDA package in misc/chamfer.py; nothing of it is used here).

    a_to_b, b_to_a = chamfer_distance(a, b)                       # (B,) each: mean squared distance to the nearest point of the other cloud
    f, precision, recall = f_score(a, b, tau=0.01)
    points, face_idx, bary = sample_surface(vertices, faces, 100_000)
    scores = reconstruction_metrics(generator, z, cloud, voxel_resolution=256)
    scores = mesh_metrics(vertices, faces, cloud)                # the same scores of any mesh, such as extract_mesh_tsdf's

The nearest-point search is ops.nearest_points (cnerf_nearest_points: exact, brute force, in HIP; include/cnerf.h states its contract);
nothing n x m is ever stored.  Everything above it is PyTorch plumbing.

chamfer_distance is differentiable in both clouds.  Its forward value is the kernel's own squared distance; the backward uses the saved
index of the nearest target: 2 g (a_i - b_idx) to the query and the negative of that added at idx to the target.  The add at idx is an
index_add_, whose order of additions is not fixed on the GPU: the target-side gradient is NOT bit-reproducible from run to run (the
forward values, the indices and the query-side gradient are)."""
import math

import torch

from . import _lib as L
from . import extract_shapes, ops


def _batched(a, b, what):
    """(n,3) and (m,3) -> one image; returns a (B,n,3), b (B,m,3) and whether the batch axis was added."""
    single = a.dim() == 2 and b.dim() == 2
    if single:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3 or a.shape[0] != b.shape[0]:
        raise L.CnerfError(f"{what}: the clouds must be (B,n,3) and (B,m,3) (or (n,3) and (m,3)), got {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b, single


def _lengths(lengths, B, full, dev):
    """Per-image lengths clamped to [0, full] as int64 (B,) on dev; None: all rows."""
    if lengths is None:
        return torch.full((B,), full, dtype=torch.int64, device=dev)
    return torch.as_tensor(lengths).detach().to(device=dev, dtype=torch.int64).reshape(B).clamp(0, full)


def _search(a, b, a_len, b_len):
    """ops.nearest_points, or (+inf, -1) without a launch where a cloud has no rows at all."""
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    if n == 0 or m == 0:
        return (torch.full((B, n), math.inf, dtype=torch.float32, device=a.device), torch.full((B, n), -1, dtype=torch.int32, device=a.device))
    return ops.nearest_points(a, b, a_len, b_len)


class _NearestDist2(torch.autograd.Function):
    """dist2 (B,n) of ops.nearest_points as an autograd node over both clouds."""

    @staticmethod
    def forward(ctx, a, b, a_len, b_len):
        dist2, idx = _search(a, b, a_len, b_len)
        ctx.save_for_backward(a, b, idx)
        ctx.mark_non_differentiable(idx)
        return dist2, idx

    @staticmethod
    def backward(ctx, g, _):
        a, b, idx = ctx.saved_tensors
        B, m = b.shape[0], b.shape[1]
        chosen = idx >= 0
        j = idx.clamp(min=0).long()
        nearest = torch.gather(b, 1, j.unsqueeze(-1).expand(-1, -1, 3)) if m else torch.zeros_like(a)
        # rows without a chosen target (idx = -1: beyond the length, an empty or all non-finite target side) get exactly zero
        ga = torch.where(chosen.unsqueeze(-1), 2.0 * g.unsqueeze(-1) * (a - nearest).to(g.dtype), torch.zeros((), dtype=g.dtype, device=g.device))
        gb = None
        if ctx.needs_input_grad[1]:
            gb = torch.zeros((B * m, 3), dtype=ga.dtype, device=ga.device)
            if m:
                flat = (j + torch.arange(B, device=j.device).unsqueeze(1) * m).reshape(-1)
                gb.index_add_(0, flat, -ga.reshape(-1, 3))          # order of additions not fixed: see the module's docstring
            gb = gb.reshape(B, m, 3).to(b.dtype)
        return (ga.to(a.dtype) if ctx.needs_input_grad[0] else None), gb, None, None


def _direction(a, b, a_len, b_len, squared):
    """Mean over the valid rows of a of the (squared) distance to the nearest valid row of b -> (B,); nan where either side is empty."""
    d2, _ = _NearestDist2.apply(a, b, a_len, b_len)
    n = a.shape[1]
    ok = (a_len > 0) & (b_len > 0)
    rows = (torch.arange(n, device=a.device).unsqueeze(0) < a_len.unsqueeze(1)) & ok.unsqueeze(1)
    if squared:
        d = d2
    else:       # the root's slope at 0 is unbounded: coincident points take the subgradient 0
        pos = d2 > 0
        d = torch.where(pos, torch.where(pos, d2, torch.ones_like(d2)).sqrt(), torch.zeros_like(d2))
    # the terms are the kernel's fp32 values; they are summed in float64 so that the mean is their correctly rounded mean
    total = torch.where(rows, d, torch.zeros_like(d)).double().sum(1)
    mean = (total / a_len.clamp(min=1).double()).to(d2.dtype)
    return torch.where(ok, mean, torch.full_like(mean, math.nan))


def chamfer_distance(a, b, a_lengths=None, b_lengths=None, squared=True):
    """The two directed Chamfer terms of clouds a (B,n,3) and b (B,m,3): a_to_b[i] = mean over a's valid rows of the squared distance
    to the nearest valid row of b, b_to_a the reverse -> two (B,) tensors (0-dim for (n,3) and (m,3) inputs).  a_lengths / b_lengths
    (B,): how many leading rows of each image count.  squared=False: the root of each distance is taken before the mean.
    Differentiable in a and b (see the module's docstring; the gradient to the side that plays the target is not bit-reproducible).
    An image with an empty side gives nan in both directions and contributes no gradient.  The symmetric Chamfer distance of the
    literature is a_to_b + b_to_a."""
    a, b, single = _batched(a, b, "chamfer_distance")
    if a.dtype != torch.float32:
        a = a.float()
    if b.dtype != torch.float32:
        b = b.float()
    a, b = a.contiguous(), b.contiguous()
    B = a.shape[0]
    a_len, b_len = _lengths(a_lengths, B, a.shape[1], a.device), _lengths(b_lengths, B, b.shape[1], a.device)
    ab = _direction(a, b, a_len, b_len, squared)
    ba = _direction(b, a, b_len, a_len, squared)
    return (ab[0], ba[0]) if single else (ab, ba)


def f_score(a, b, tau, a_lengths=None, b_lengths=None):
    """F-score at threshold tau (unsquared distance): precision = the share of a's valid points within tau of b, recall = the share of
    b's within tau of a, f = 2 p r / (p + r), 0 where p + r == 0 -> (f, precision, recall), (B,) each (0-dim for unbatched inputs).
    Not differentiable.  An image with an empty side gives nan."""
    a, b, single = _batched(a, b, "f_score")
    B = a.shape[0]
    a_len, b_len = _lengths(a_lengths, B, a.shape[1], a.device), _lengths(b_lengths, B, b.shape[1], a.device)
    ok = (a_len > 0) & (b_len > 0)

    def share(x, y, x_len, y_len):
        with torch.no_grad():
            d2, _ = _search(ops._f32(x.detach()), ops._f32(y.detach()), x_len, y_len)
        rows = torch.arange(x.shape[1], device=x.device).unsqueeze(0) < x_len.unsqueeze(1)
        within = (d2.sqrt() <= float(tau)) & rows
        return within.sum(1).double() / x_len.clamp(min=1).double()

    p, r = share(a, b, a_len, b_len), share(b, a, b_len, a_len)
    s = p + r
    f = torch.where(s > 0, 2 * p * r / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    nan = torch.full_like(f, math.nan)
    out = tuple(torch.where(ok, v, nan).float() for v in (f, p, r))
    return tuple(v[0] for v in out) if single else out


def sample_surface(vertices, faces, n, u=None, generator=None, attrs=None):
    """n points on a triangle mesh, uniform in area.  vertices (Nv,3), faces (Nt,3) integer, attrs (Nv,C) optional per-vertex values.
    -> points (n,3), face_idx (n,) int64, bary (n,3)[, attrs (n,C) interpolated with bary].  Pure torch, on the device of `vertices`
    (the CPU included).

    u (n,3) in [0,1) makes the draw reproducible; otherwise it is torch.rand under `generator`.  Triangle areas are fp32, their
    cumulative sum float64; the triangle of a draw is searchsorted(cum, u0 * total, right=True), clamped to the last triangle of
    non-zero area, so a zero-area triangle (the isosurface keeps those) is never drawn.  With s = sqrt(u1) the barycentric weights are
    (1 - s, s (1 - u2), s u2).  ValueError: no faces, or no face of non-zero area."""
    vertices = vertices.detach()
    if vertices.dtype != torch.float32:
        vertices = vertices.float()
    dev = vertices.device
    faces = faces.detach().to(device=dev, dtype=torch.int64)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"sample_surface: vertices must be (Nv,3) and faces (Nt,3), got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    n = int(n)
    if u is None:
        u = torch.rand((n, 3), generator=generator, device=dev, dtype=torch.float32)
    else:
        u = torch.as_tensor(u).detach().to(device=dev, dtype=torch.float32)
        if tuple(u.shape) != (n, 3):
            raise ValueError(f"sample_surface: u must be ({n},3), got {tuple(u.shape)}")
    corners = vertices[faces]                                              # (Nt,3,3)
    area = 0.5 * torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).norm(dim=1)
    live = torch.nonzero(area > 0).reshape(-1)
    if live.numel() == 0:
        raise ValueError("sample_surface: the mesh has no triangle of non-zero area")
    cum = torch.cumsum(area.double(), 0)
    k = torch.searchsorted(cum, u[:, 0].double() * cum[-1], right=True).clamp(max=int(live[-1]))
    s = u[:, 1].sqrt()
    bary = torch.stack([1 - s, s * (1 - u[:, 2]), s * u[:, 2]], 1)
    tri = faces[k]                                                         # (n,3)
    mix = lambda values: bary[:, 0:1] * values[tri[:, 0]] + bary[:, 1:2] * values[tri[:, 1]] + bary[:, 2:3] * values[tri[:, 2]]
    points = mix(vertices)
    if attrs is None:
        return points, k, bary
    attrs = attrs.detach().to(device=dev, dtype=torch.float32)
    return points, k, bary, mix(attrs)


METRIC_KEYS = ("chamfer_mesh_to_cloud", "chamfer_cloud_to_mesh", "chamfer", "f_score", "precision", "recall")


def mesh_metrics(vertices, faces, cloud, n_samples=100_000, tau=0.01, u=None, return_samples=False):
    """How far a triangle mesh lies from a point cloud: n_samples area-weighted points of the mesh (sample_surface; u (n_samples,3) fixes
    the draw), then chamfer_distance (squared) and f_score at tau between those samples and cloud[..., :3] ((N,>=3) or (1,N,>=3); further
    columns, such as colours, are ignored).  vertices (Nv,3) and faces (Nt,3) on the GPU, as ops.isosurface returns them: a density mesh
    (extract_mesh) and a TSDF mesh (extract_mesh_tsdf) are scored by the same code.
    -> dict of Python floats: chamfer_mesh_to_cloud, chamfer_cloud_to_mesh, chamfer (their sum), f_score, precision (of the mesh's
    samples), recall (of the cloud), and the ints vertices, triangles.  An empty mesh gives nan metrics and zero counts.
    return_samples=True: (dict, samples (n_samples,3) on the device; (0,3) for an empty mesh)."""
    cloud = torch.as_tensor(cloud).detach().to(device=vertices.device, dtype=torch.float32)
    if cloud.dim() == 3 and cloud.shape[0] == 1:
        cloud = cloud[0]
    if cloud.dim() != 2 or cloud.shape[-1] < 3:
        raise L.CnerfError(f"mesh_metrics: cloud must be (N,>=3) or (1,N,>=3), got {tuple(cloud.shape)}")
    cloud = cloud[:, :3].contiguous()
    out = {k: math.nan for k in METRIC_KEYS}
    out["vertices"], out["triangles"] = int(vertices.shape[0]), int(faces.shape[0])
    samples = vertices.new_zeros((0, 3))
    if faces.shape[0] > 0 and cloud.shape[0] > 0:
        samples = sample_surface(vertices, faces, n_samples, u=u)[0]
        with torch.no_grad():
            ab, ba = chamfer_distance(samples, cloud)
            f, p, r = f_score(samples, cloud, tau)
        out.update(chamfer_mesh_to_cloud=float(ab), chamfer_cloud_to_mesh=float(ba), chamfer=float(ab) + float(ba), f_score=float(f),
                   precision=float(p), recall=float(r))
    return (out, samples) if return_samples else out


def reconstruction_metrics(generator, z, cloud, voxel_resolution=128, cube_length=1.2, level=10.0, n_samples=100_000, tau=0.01, u=None,
                           return_samples=False):
    """How far the surface of one conditioned scene lies from a point cloud (the one it was conditioned on): extract_mesh at `level`,
    then mesh_metrics of that mesh against the cloud, which states the samples, the scores and what is returned.  Floaters are
    sampled by area like the object and count against both scores: to score the object alone, mesh_metrics of
    extract_mesh(..., keep_largest=True)."""
    vertices, faces, _ = extract_shapes.extract_mesh(generator, z, voxel_resolution=voxel_resolution, cube_length=cube_length, level=level, colors=False)
    return mesh_metrics(vertices, faces, cloud, n_samples=n_samples, tau=tau, u=u, return_samples=return_samples)
