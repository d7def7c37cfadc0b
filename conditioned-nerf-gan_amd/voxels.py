"""The conditioning voxel grid of a coloured point cloud, made on the device, and its picture.

The reference prepares the grid offline (feature_volume/pcl2voxel.py: open3d's VoxelGrid and a Python loop over its voxels, one file per
resolution -- voxel.npz, voxel_32.npz, voxel_128.npz, read at datasets.py:131-157) and pictures it with feature_volume/voxel2img.py.
Here one cloud serves every voxel_resolution, the script's noise_xyz / noise_color augmentation is a per-call option, and the grid the
encoder sees is made from the same cloud that shape_metrics scores against.  The kernels are cnerf_voxelize and cnerf_voxel_first_hit
(include/cnerf.h states both contracts); everything here is forward only."""
import numpy as np
import torch

from . import ops
from .generators.volumetric_rendering import pinhole_rays

CLIP_MARGIN = 1e-4      # pcl2voxel.py:40


def voxelize_cloud(pcl, resolution=64, length=1.2, noise_xyz=0.0, noise_color=0.0, generator=None, lengths=None):
    """pcl (B,n,6 or more) = [x, y, z, r, g, b, ...] on the GPU (or (n,6) for one cloud) -> (B,4,V,V,V) = [occupancy, r, g, b] indexed
    [b, ch, iz, iy, ix] over the cube [-length/2, length/2]^3, V = resolution: what the 3D U-Net takes.
    The steps of pcl2voxel.py:38-41 in their order: Gaussian noise of standard deviation noise_xyz on the positions and noise_color on
    the colours (torch.randn on the device, from `generator` if given; nothing is drawn for a deviation of 0), positions clipped into
    [-length/2 + 1e-4, length/2 - 1e-4], colours into [0,1]; then a cell is occupied where a point fell and holds the mean colour of
    its points.  lengths (B,): how many leading rows of each cloud count.  The output carries no gradient."""
    pcl = pcl.detach()
    if noise_xyz or noise_color:
        pcl = pcl[..., :6].float()
        shape = pcl.shape[:-1] + (3,)
        xyz, rgb = pcl[..., :3], pcl[..., 3:6]
        if noise_xyz:
            xyz = xyz + torch.randn(shape, device=pcl.device, generator=generator) * float(noise_xyz)
        if noise_color:
            rgb = rgb + torch.randn(shape, device=pcl.device, generator=generator) * float(noise_color)
        pcl = torch.cat([xyz, rgb], -1)
    return ops.voxelize(pcl, int(resolution), -float(length) / 2, float(length), lengths=lengths, clip_margin=CLIP_MARGIN, layout="encoder")


def voxel_surface_render(voxels, cam2worlds, img_size, fov, ray_start, ray_end, num_steps=256, length=1.2):
    """The picture of a voxel grid (voxel2img.voxel_surface_render): voxels (B,4,V,V,V) as the encoder takes them, one camera (B,4,4) per
    grid -> (B,3,R,R), R = img_size.  Per pixel of the pinhole grid the colour of the first occupied voxel among num_steps samples of
    [ray_start, ray_end] along its ray, white where there is none; colours in the grid's own range.  A sample outside the cube sees
    nothing: the reference's border padding, which smears the border voxels over all of space, is not reproduced."""
    R = int(img_size)
    origins, dirs = pinhole_rays(cam2worlds, R, fov)
    pixels, _, _ = ops.voxel_first_hit(voxels, origins, dirs, -float(length) / 2, float(length), ray_start, ray_end, num_steps,
                                       background=(1.0, 1.0, 1.0), layout="encoder")
    return pixels.reshape(voxels.shape[0], R, R, 3).permute(0, 3, 1, 2).contiguous()


def save_voxel_npz(path, voxels_one_image, length, noise_xyz=0, noise_color=0):
    """Writes the reference's voxel file (pcl2voxel.py:60-74) from one grid (4,V,V,V) indexed [ch, iz, iy, ix]: 'voxel' (X,Y,Z,4)
    float64, 'length', 'resolution', 'noise_color', 'noise_xyz'.  training.formats.load_voxel_npz reads it back to the same values."""
    v = voxels_one_image.detach()
    if v.dim() != 4 or v.shape[0] != 4 or not (v.shape[1] == v.shape[2] == v.shape[3]):
        raise ValueError(f"save_voxel_npz: expected one grid (4,V,V,V), got {tuple(v.shape)}")
    voxel = np.ascontiguousarray(v.permute(3, 2, 1, 0).cpu().numpy().astype(np.float64))
    np.savez(path, length=length, resolution=int(v.shape[1]), noise_color=noise_color, noise_xyz=noise_xyz, voxel=voxel)
