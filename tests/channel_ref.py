"""Shared by tests/test_channel.py and tests/test_channel_gpu.py: the problems and the command-line case of the channel / label
reconstruction (csrc/svr_channel.inc; --channelStacks / --labelStacks / --manualMask of csrc/svr_cli.cpp), and the reader of the command
line's --dumpChannels file."""
import numpy as np


def awkward_problem():
    """3 stacks of 37 x 29 x 7 with the default slice motion, one stack turned 30 degrees in its plane, in a volume of 31^3: the slice
    grid (37 * 29 * 21 = 22533 pixels) and nv (29791) are multiples of neither 4 nor 64, the slices are oblique."""
    from fetalreconstruction_amd import phantom
    return phantom.make_problem(n_stacks=3, stack_shape=(37, 29, 7), in_plane=1.1, spacing=2.2, recon_res=1.0, mask_radius=12.4, seed=7,
                                orientations=("ax30", "cor", "sag"), name="channel-awkward")


def case_stacks():
    """the tiny phantom as stacks: three of 32 x 32 x 8, no stack motion (as tests/slice_quality_ref.py's, uncorrupted)"""
    from fetalreconstruction_amd import phantom
    stacks, mask, mattr, rattr, rmask = phantom.make_stacks(3, (32, 32, 8), 1.1, 2.2, None, 1.0, 14.0, seed=1, orientations=("ax", "cor", "sag"),
                                                            stack_motion_mm=0.0, stack_motion_deg=0.0)
    return stacks, rattr, rmask


def write_cli_case(d, stacks=None, rattr=None, rmask=None):
    """the stacks and the mask as files -> (the common arguments of the command line, the stacks' paths, the stacks)"""
    from fetalreconstruction_amd import nifti
    if stacks is None:
        stacks, rattr, rmask = case_stacks()
    paths = []
    for k, st in enumerate(stacks):
        nifti.write(d / f"stack{k}.nii.gz", st.data, st.attr)
        paths.append(str(d / f"stack{k}.nii.gz"))
    nifti.write(d / "mask.nii.gz", rmask, rattr)
    args = ["-i", *paths, "-m", str(d / "mask.nii.gz"), "--thickness", "2.2", "2.2", "2.2", "--resolution", "1.0", "--no_registration",
            "--iterations", "1", "--rec_iterations_last", "5", "--smooth_mask", "0"]
    return args, paths, stacks


def write_like(d, name, stacks, fn):
    """fn(k, stack) -> an array on stack k's grid (or None: `none`), written next to the stacks -> the file names for the command line"""
    from fetalreconstruction_amd import nifti
    out = []
    for k, st in enumerate(stacks):
        a = fn(k, st)
        if a is None:
            out.append("none")
            continue
        p = d / f"{name}{k}.nii.gz"
        nifti.write(p, np.asarray(a, np.float32), st.attr)
        out.append(str(p))
    return out


def pixel_world(attr):
    """world coordinates of every voxel centre of an image, [nz][ny][nx][3]"""
    from fetalreconstruction_amd import geometry as geo
    kk, jj, ii = np.meshgrid(np.arange(attr.nz), np.arange(attr.ny), np.arange(attr.nx), indexing="ij")
    pix = np.stack([ii, jj, kk, np.ones_like(ii)], -1).astype(np.float64)
    return (pix @ geo.image_to_world(attr).T)[..., :3]


def read_channel_dump(path):
    """--dumpChannels -> [(labels?, unit_on uint8 [ns], grid float32 [ns][my][mx], label values float32)]"""
    raw = open(path, "rb").read()
    nsets, ns, mx, my = (int(v) for v in np.frombuffer(raw, np.int32, 4))
    o, out = 16, []
    for _ in range(nsets):
        labels, nl = (int(v) for v in np.frombuffer(raw, np.int32, 2, o)); o += 8
        unit_on = np.frombuffer(raw, np.uint8, ns, o); o += ns
        grid = np.frombuffer(raw, np.float32, ns * my * mx, o).reshape(ns, my, mx); o += 4 * ns * my * mx
        vals = np.frombuffer(raw, np.float32, nl, o); o += 4 * nl
        out.append((bool(labels), unit_on, grid, vals))
    assert o == len(raw)
    return out


def read_problem_dump(path, n_stacks):
    """--dumpProblem (the format of csrc/svr_cli.cpp, version 2) -> dict(ns, mx, my, vsize, attrs of the cropped stacks as raw float64 rows,
    grid [ns][my][mx], factors, sizes_x, sizes_y)"""
    raw = open(path, "rb").read()
    ns, mx, my, n, vx, vy, vz, ver = (int(v) for v in np.frombuffer(raw, np.int32, 8))
    assert n == n_stacks and ver == 2
    ATTR = 16 + 15 * 8                                   # struct svr_image_attr: three ints (padded to 16 bytes), fifteen doubles
    o = 32 + ATTR + 8 * vx * vy * vz
    attrs = []
    for _ in range(n):
        dims = np.frombuffer(raw, np.int32, 3, o)
        dbl = np.frombuffer(raw, np.float64, 15, o + 16)
        attrs.append((tuple(int(v) for v in dims), dbl.copy()))
        o += ATTR
    grid = np.frombuffer(raw, np.float32, ns * my * mx, o).reshape(ns, my, mx); o += 4 * ns * my * mx
    o += 8 * 16 * ns
    factors = np.frombuffer(raw, np.float32, n, o); o += 4 * n
    sizes_x = np.frombuffer(raw, np.int32, ns, o); o += 4 * ns
    sizes_y = np.frombuffer(raw, np.int32, ns, o); o += 4 * ns
    assert o == len(raw)
    return dict(ns=ns, mx=mx, my=my, vsize=(vx, vy, vz), attrs=attrs, grid=grid, factors=factors, sizes_x=sizes_x, sizes_y=sizes_y)
