"""Between rendered views and shapes, on the device: depth maps fused into one coloured cloud or into a truncated signed distance volume
(tsdf_volume: cnerf_tsdf_integrate, whose zero level extract_shapes.extract_mesh_tsdf meshes), and the z-buffered picture of a cloud.

The reference looks at a scene's geometry with Inferencer.render_pcl (inference.py:501-601): it renders n views, lifts every pixel whose
depth lies strictly inside (ray_start, ray_end) into world space on the host -- nonzero, indexing, a 4x4 matmul per view in a Python
loop -- colours it and writes an .obj.  Its render_pcl_masked and its loss_depth (utils.py:96-99) need a ground-truth depth image per
camera, which it reads from EXR files.  Here the lift is one kernel over all views (cnerf_backproject), the cloud it returns goes
straight into shape_metrics and voxels.voxelize_cloud, and the depth image of the cloud a scene was conditioned on comes from
cnerf_splat_points.  include/cnerf.h states both contracts; everything here is forward only."""
import numpy as np
import torch

from . import ops


def focal_of(fov):
    """1 / tan(fov / 2) in fp32, formed as volumetric_rendering.pinhole_rays and the render kernels form it (2.187719 at 49.13 degrees;
    the reference's reprojection uses the literal 2.1875)."""
    return float(np.float32(1.0) / np.float32(np.tan((2 * np.pi * fov / 360) / 2)))


def fuse_depth_maps(pixels, depth, cam2worlds, fov, ray_start, ray_end, mask=None):
    """Rendered views -> one cloud: pixels (V,3,R,R) in [-1,1] and depth (V,R,R) as the generator returns them, cam2worlds (V,4,4).
    Every pixel with ray_start < depth < ray_end (and mask > 1e-4 where mask (V,R,R) is given, render_pcl_masked's rule) becomes a
    point [x, y, z, r, g, b] in world space, colours 0.5 * pixels + 0.5, in ascending (view, row, col) -> (n,6) float32."""
    return ops.backproject(depth, cam2worlds, focal_of(fov), ray_start, ray_end, colors=pixels, color_layout="chw", color_scale=0.5, color_offset=0.5,
                           mask=mask, mask_min=1e-4)[0]


def render_views(gen, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, views_per_batch=None, **render_kwargs):
    """Renders ONE scene z (batch 1, as the generator takes it: a feature volume, a (volume, global feature) pair or a latent) from the
    cameras cam2worlds (V,4,4) under no_grad, views_per_batch at a time (None: all at once).  render_kwargs go to the generator's
    forward (hierarchical_sample, clamp_mode, nerf_noise, ...).  -> pixels (V,3,R,R), depth (V,R,R)."""
    V = int(cam2worlds.shape[0])
    step = V if views_per_batch is None else max(1, int(views_per_batch))

    def expand(t, k):
        return tuple(expand(u, k) for u in t) if isinstance(t, (tuple, list)) else t.expand(k, *t.shape[1:])

    imgs, depths = [], []
    with torch.no_grad():
        for v0 in range(0, V, step):
            cams = cam2worlds[v0:v0 + step]
            img, dep = gen(expand(z, cams.shape[0]), cams, img_size=img_size, fov=fov, ray_start=ray_start, ray_end=ray_end, num_steps=num_steps,
                           **render_kwargs)
            imgs.append(img)
            depths.append(dep)
        return torch.cat(imgs, 0), torch.cat(depths, 0)


def render_pcl(gen, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, views_per_batch=None, **render_kwargs):
    """The reference's render_pcl without the file: render_views of ONE scene z from the cameras cam2worlds (V,4,4), and the views fused
    -> (n,6).  Write it with write_obj_cloud; score it with shape_metrics; voxelise it with voxels.voxelize_cloud."""
    pixels, depth = render_views(gen, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, views_per_batch, **render_kwargs)
    with torch.no_grad():
        return fuse_depth_maps(pixels, depth, cam2worlds, fov, ray_start, ray_end)


def tsdf_volume(pixels, depth, cam2worlds, fov, ray_start, ray_end, resolution=256, cube_length=1.2, origin=(0, 0, 0), trunc=None, carve=True,
                hidden_min=1, unseen=-1.0, want_weight=False):
    """Rendered views -> a truncated signed distance volume: pixels (V,3,R,R) in [-1,1] (or None) and depth (V,R,R) as render_views returns
    them, cam2worlds (V,4,4).  The cube of edge cube_length about origin, resolution^3 lattice points: corner lo = origin - cube_length / 2,
    pitch = cube_length / (resolution - 1), lattice axis c = world axis c.  trunc=None: three pitches.  Pixels with
    ray_start < depth < ray_end are surface, all others but NaNs background (the renderer's depth of an empty ray is near 0); colours are
    0.5 * pixels + 0.5, as in fuse_depth_maps.  ops.tsdf_integrate states the rule, include/cnerf.h the arithmetic.
    -> tsdf (N,N,N), weight (int32, or None without want_weight), rgb (N,N,N,3) in [0,1] (None without pixels), lo (three floats), pitch:
    ops.isosurface(tsdf, 0.0, lo, pitch, attrs=rgb) is the mesh."""
    N = int(resolution)
    if N < 2:
        raise ValueError(f"tsdf_volume: resolution={resolution} must be at least 2")
    lo = tuple(float(o) - 0.5 * float(cube_length) for o in origin)
    pitch = float(cube_length) / (N - 1)
    trunc = 3.0 * pitch if trunc is None else float(trunc)
    tsdf, weight, rgb = ops.tsdf_integrate(depth, cam2worlds, focal_of(fov), ray_start, ray_end, (N, N, N), lo, pitch, trunc, colors=pixels,
                                           color_layout="chw", color_scale=0.5, color_offset=0.5, carve=carve, hidden_min=hidden_min, unseen=unseen,
                                           want_weight=want_weight)
    return tsdf, weight, rgb, lo, pitch


def splat_cloud(pcl, cam2worlds, img_size, fov, z_min, z_max, radius=1, lengths=None):
    """The picture of clouds from cameras: pcl (B,n,6 or more) = [x, y, z, r, g, b, ...], cam2worlds (B,V,4,4) -- or (B,4,4): V = 1.
    -> image (B,V,3,R,R) in the cloud's own colour range, white where nothing landed; depth (B,V,R,R), the camera-space z of the
    nearest point, 0 = background (what loss_depth and the reference's masks expect); index (B,V,R,R) int32, that point's row or -1.
    A point covers (2 radius + 1)^2 pixels.  The picture of a SPARSE cloud is a proxy of the surface's: where the footprints do not
    close the surface a pixel sees the far side of the object, so radius must suit the cloud's density at this image size."""
    if cam2worlds.dim() == 3:
        cam2worlds = cam2worlds.unsqueeze(1)
    depth, index, pixels = ops.splat_points(pcl, cam2worlds, int(img_size), focal_of(fov), z_min, z_max, radius=radius, lengths=lengths,
                                            background=(1.0, 1.0, 1.0), want_pixels=True)
    return pixels.permute(0, 1, 4, 2, 3).contiguous(), depth, index


def write_obj_cloud(path, cloud):
    """The reference's coloured .obj (inference.py:562-590): one line `v x y z r g b` per row of cloud (n,6), positions as str(float32),
    colours as uchar by its rule: c * 255 + 0.5, clamped to [0,255], truncated."""
    c = cloud.detach().cpu().numpy() if torch.is_tensor(cloud) else np.asarray(cloud)
    c = np.ascontiguousarray(c, np.float32)
    if c.ndim != 2 or c.shape[1] < 6:
        raise ValueError(f"write_obj_cloud: expected a cloud (n,6), got {c.shape}")
    rgb = np.clip(c[:, 3:6] * np.float32(255) + np.float32(0.5), 0, 255).astype("uint8")
    with open(path, "w") as f:
        for p, k in zip(c, rgb):
            f.write("v " + " ".join(str(x) for x in (p[0], p[1], p[2], k[0], k[1], k[2])) + "\n")
