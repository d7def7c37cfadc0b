"""Dense density grid of a conditioned field -- the second consumer of the siren sub-API (counterpart of the reference's
extract_shapes.py:15-78; that file itself imports mrcfile / plyfile, which this image lacks, so its numbers are restated
here, not pinned: the grid arithmetic below is written to give the same sample coordinates).

    sigma = sample_generator(generator, z, voxel_resolution=256)        # (N, N, N) numpy array, sigma[i0, i1, i2]

The field kernel takes the whole grid in a few launches (2^22 points per call) instead of the reference's 64^3 slices.

The surface itself, which the reference leaves to outside tools:

    vertices, faces, colors = extract_mesh(generator, z, voxel_resolution=256)     # device tensors: (Nv,3), (Nt,3) int32, (Nv,3)
    write_ply("car.ply", vertices, faces, colors)

extract_mesh keeps the grid's four field channels on the device and hands them to ops.isosurface (marching tetrahedra in HIP,
include/cnerf.h states the algorithm); nothing but the two counts crosses to the host.

A mesh without a density level to guess, from the rendered depth of a ring of views fused into a TSDF volume (cnerf_tsdf_integrate):

    vertices, faces, colors = extract_mesh_tsdf(generator, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps)"""
import numpy as np
import torch

from . import ops


def create_samples(N=256, voxel_origin=(0, 0, 0), cube_length=2.0):
    """(1, N^3, 3) sample coordinates, the corner of the cube and the voxel pitch.

    Point n of the flat grid has column 2 = n mod N and columns 1, 0 = (n / N) mod N, (n / N^2) mod N evaluated in floating
    point WITHOUT flooring -- the reference's convention (extract_shapes.py:24-27), kept so that grids line up with grids
    extracted by it; each column is then scaled by the pitch and shifted by the cube corner (columns 0 / 2 take the corner's
    components 2 / 0: the corner is symmetric in practice)."""
    corner = np.asarray(voxel_origin, dtype=np.float64) - cube_length / 2
    pitch = cube_length / (N - 1)
    n = torch.arange(N ** 3, dtype=torch.int64)
    nf = n.float()
    pts = torch.empty(N ** 3, 3)
    pts[:, 2] = (n % N).float() * pitch + float(corner[0])
    pts[:, 1] = ((nf / N) % N) * pitch + float(corner[1])
    pts[:, 0] = (((nf / N) / N) % N) * pitch + float(corner[2])
    return pts.unsqueeze(0), corner, pitch


def sample_generator(generator, z, voxel_resolution=256, voxel_origin=(0, 0, 0), cube_length=1.2, psi=0.5, max_points=1 << 22):
    """sigma on the N^3 grid as a (N, N, N) numpy array (extract_shapes.py:41-78; `psi` is accepted and unused there too)."""
    N = int(voxel_resolution)
    pts, _, _ = create_samples(N, voxel_origin, cube_length)
    pts = pts.to(generator.device)
    sig = torch.empty((1, N ** 3), dtype=torch.float32, device=generator.device)
    with torch.no_grad():
        for s0 in range(0, N ** 3, max_points):
            chunk = pts[:, s0:s0 + max_points].contiguous()
            sig[:, s0:s0 + chunk.shape[1]] = generator.siren(chunk, z, N, 1)[..., 3]
    return sig.reshape(N, N, N).cpu().numpy()


def extract_mesh(generator, z, voxel_resolution=256, voxel_origin=(0, 0, 0), cube_length=1.2, level=0.0, colors=True, max_points=1 << 22,
                 keep_largest=False, min_component=0):
    """The level set sigma = level of one conditioned scene as an indexed triangle mesh on the device: vertices (Nv,3) float32, faces
    (Nt,3) int32, colors (Nv,3) float32 (the field's channels 0..2 interpolated along the crossed edges) or None.

    The grid is sample_generator's (same coordinates, same chunking).  Lattice point (i0,i1,i2) is given the position
    i_c * pitch + (corner[2], corner[1], corner[0])[c] -- create_samples' column convention; its columns 0 and 1 are not floored, so off
    the i2 = 0 face the field is sampled up to one pitch beyond that position on those axes, as in every grid the reference extracts.
    The normals point toward falling sigma: out of the shape.

    keep_largest / min_component: every blob of density above the level is a closed sheet of its own (a floater).  With keep_largest only
    the largest connected solid is meshed, with min_component = k only solids of at least k lattice points (ops.keep_components on the very
    lattice the isosurface reads, so its axes are the split's): what is left is, bit for bit, part of the unfiltered mesh."""
    N = int(voxel_resolution)
    pts, corner, pitch = create_samples(N, voxel_origin, cube_length)
    pts = pts.to(generator.device)
    field = torch.empty((1, N ** 3, 4), dtype=torch.float32, device=generator.device)
    with torch.no_grad():
        for s0 in range(0, N ** 3, max_points):
            chunk = pts[:, s0:s0 + max_points].contiguous()
            field[:, s0:s0 + chunk.shape[1]] = generator.siren(chunk, z, N, 1)
    field = field.reshape(N, N, N, 4)
    sigma = field[..., 3].contiguous()
    attrs = field[..., :3].contiguous() if colors else None
    lo = (float(corner[2]), float(corner[1]), float(corner[0]))
    if keep_largest or min_component > 0:
        sigma = ops.keep_components(sigma, level, largest=keep_largest, min_size=min_component)
    return ops.isosurface(sigma, level, lo=lo, pitch=pitch, attrs=attrs)


def extract_mesh_tsdf(generator, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, voxel_resolution=256, cube_length=1.2,
                      voxel_origin=(0, 0, 0), trunc=None, colors=True, views_per_batch=None, **render_kwargs):
    """The surface the RENDERED DEPTH of one conditioned scene describes, with no density threshold to guess: views.render_views from the
    cameras cam2worlds (V,4,4), views.tsdf_volume of the depth maps over the cube of edge cube_length about voxel_origin, and the zero
    level of that volume by ops.isosurface.  -> vertices (Nv,3) float32, faces (Nt,3) int32, colors (Nv,3) float32 in [0,1] (the mean of
    the rendered pixels that saw the surface; None with colors=False), device tensors like extract_mesh's, ready for write_ply.  Here
    lattice axis c is world axis c (not extract_mesh's reversed columns), and the normals point out of the shape.

    What to choose.  Cameras all around the object: a side no view looks at is closed by the visual hull of the others, not by its own
    depth.  A cube no larger than the views cover: a voxel that only a view or two see, behind the object, counts as solid (the hidden
    rule, include/cnerf.h) and shows as a blob in a corner of the cube.  trunc (None: three pitches) of at least two or three pitches:
    with less, the inside end of a crossed edge may lie beyond the band in every view and have no colour (it then pulls the vertex's
    colour toward black), and the surface follows single pixels.

    render_kwargs go to the generator's forward, but for four keywords that are taken out of them first (this function's parameter
    list is fixed): hidden_min=1, keep_largest=False, min_component=0, fill_cavities=False.  hidden_min is views.tsdf_volume's.  The
    others are for what more cameras or a smaller cube do not cure.  keep_largest meshes only the largest connected solid, and
    min_component = k only solids of at least k lattice points: the blobs in the cube's corners go.  fill_cavities keeps the largest
    connected free region, the one around the object, and makes every other one solid: the second, inner surface of a volume without
    the hidden rule goes.  The solids are filtered first, then the cavities, by ops.keep_components on the volume the isosurface reads;
    the fills are -1 and +1, the volume's own free and solid values, and what is left of the mesh is bit for bit part of the unfiltered
    one."""
    from . import views
    hidden_min, keep_largest = render_kwargs.pop("hidden_min", 1), render_kwargs.pop("keep_largest", False)
    min_component, fill_cavities = render_kwargs.pop("min_component", 0), render_kwargs.pop("fill_cavities", False)
    pixels, depth = views.render_views(generator, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, views_per_batch, **render_kwargs)
    tsdf, _, rgb, lo, pitch = views.tsdf_volume(pixels if colors else None, depth, cam2worlds, fov, ray_start, ray_end, resolution=voxel_resolution,
                                                cube_length=cube_length, origin=voxel_origin, trunc=trunc, hidden_min=hidden_min)
    if keep_largest or min_component > 0:
        tsdf = ops.keep_components(tsdf, 0.0, largest=keep_largest, min_size=min_component, fill=-1.0)
    if fill_cavities:
        tsdf = ops.keep_components(tsdf, 0.0, largest=True, fill=1.0, invert=True)
    return ops.isosurface(tsdf, 0.0, lo=lo, pitch=pitch, attrs=rgb)


def write_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY: float x y z per vertex (and uchar red green blue = clamp(rgb, 0, 1) * 255 when colors is given), one
    uchar count + three int indices per face.  Takes tensors on any device or NumPy arrays."""
    as_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = as_np(vertices).astype("<f4").reshape(-1, 3)
    f = as_np(faces).astype("<i4").reshape(-1, 3)
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    names = ["property float x", "property float y", "property float z"]
    if colors is not None:
        props += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        names += ["property uchar red", "property uchar green", "property uchar blue"]
    vert = np.empty(len(v), dtype=props)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = (np.clip(as_np(colors).astype(np.float32).reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", *names, f"element face {len(f)}",
              "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())
