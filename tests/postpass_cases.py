"""The cases tests/test_postpass_cpu.py and tests/test_gpu_postpass.py share for the cross-cube post-pass's kernel paths that depend on the cube
width Dc (surfacenet_amd/csrc/crosscube.h): per case the seeded lists, the CPU restatement's results (tests/postpass_ref.py), computed once per
process and read-only from then on, and the one comparison both files use. tools/gen_golden_postpass.py records the same cases, on GOLDEN_LATTICE
where the table's lattice would not fit the fixture, from the reference into tests/golden/postpass_edge_cases.npz."""
import functools

import numpy as np

import postpass_ref as ref
from surfacenet_amd import synthetic

LIST_KEYS = ("prediction_list", "rgb_list", "vxl_ijk_list", "rayPooling_votes_list")
ARGS = dict(N_refine_iter=2, init_probThresh=0.5, max_probThresh=0.9, rayPool_thresh=4, beta=2)
DENOISE_PROB = 0.7          # the denoise tests' mask: pred >= 0.7 & votes >= rayPool_thresh

# name -> D_cube, Dc, lattice, thickness, amplitude, seed                                  reaches
TABLE = {
    "w27": (27, 27, (3, 2, 2), 3, 3.0, 3),          # first size with union-find parents in global memory; odd, h = 13
    "w53": (53, 53, (3, 2, 2), 3, 3.0, 3),          # first size whose three grids take two passes
    "w63": (63, 63, (3, 2, 2), 3, 3.0, 3),          # last two-pass size; odd, h = 31
    "w64": (64, 64, (3, 2, 2), 3, 3.0, 3),          # one grid per pass; bit 63 of a row; shifts by 32
    "crop32": (32, 27, (3, 2, 2), 3, 3.0, 3),       # D_cube > Dc, global parents
    "crop64": (64, 58, (3, 2, 2), 3, 3.0, 2),       # D_cube > Dc, two passes
    "tiny": (6, 5, (4, 4, 3), 2, 1.0, 3),           # rows of a few bits
    "far": (55, 27, (3, 2, 2), 3, 3.0, 3),          # D_cube = 2 Dc + 1, h >= Dc: no voxel of two cubes coincides, AND = 0 on every face
}
# the fixture holds the wide cases on fewer cubes (tests/golden/postpass_edge_cases.npz stays near the size of postpass_cases.npz)
GOLDEN_LATTICE = {"w53": (2, 1, 1), "w63": (1, 1, 2), "w64": (2, 2, 1), "crop64": (1, 2, 2)}


def mixed_votes(d, seed):
    """votes that pass rayPool_thresh = 4 for about a third of the voxels, independently per cube: the overlap of neighbours then thins
    out at the margin and the three threshold perturbations compete"""
    rs = np.random.RandomState(seed)
    d["rayPooling_votes_list"] = [np.where(rs.rand(len(v)) < 0.35, 6, 2).astype(np.uint8) for v in d["rayPooling_votes_list"]]
    return d


def edge_case(D_cube, Dc, lattice, thickness, amplitude, seed):
    """sparse_surface at width D_cube (cubes at stride D_cube // 2); with Dc < D_cube every cube's list is centre-cropped to Dc as dense2sparse
    crops a cube (utils/sparseCubes.py:53): ijk - (D_cube - Dc) // 2, kept where 0 <= ijk < Dc; then mixed votes"""
    d = synthetic.sparse_surface(lattice, D_cube, thickness=thickness, amplitude=amplitude, seed=seed)
    if Dc < D_cube:
        o = (D_cube - Dc) // 2
        for c, ijk in enumerate(d["vxl_ijk_list"]):
            loc = ijk.astype(np.int64) - o
            keep = np.all((loc >= 0) & (loc < Dc), axis=1)
            for k in LIST_KEYS:
                d[k][c] = d[k][c][keep]
            d["vxl_ijk_list"][c] = loc[keep].astype(np.uint8)
    return mixed_votes(d, seed)


def denoise_masks(d):
    return [(np.asarray(p) >= DENOISE_PROB) & (np.asarray(v) >= ARGS["rayPool_thresh"]) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]


def at_args(d, D_cube, N_refine_iter=None):
    """the positional arguments adapthresh.adapthresh_lists and postpass_ref.adapthresh_ref share"""
    return (d["prediction_list"], d["vxl_ijk_list"], d["rayPooling_votes_list"], d["cube_ijk_np"], N_refine_iter or ARGS["N_refine_iter"], D_cube,
            ARGS["init_probThresh"], ARGS["max_probThresh"], ARGS["rayPool_thresh"], ARGS["beta"])


def build(name, lattice=None):
    """the lists of a case of the table (on another lattice for the fixture) -> (d, D_cube, Dc)"""
    D_cube, Dc, lat, thickness, amplitude, seed = TABLE[name]
    d = edge_case(D_cube, Dc, lattice or lat, thickness, amplitude, seed)
    assert ref._dc(d["vxl_ijk_list"]) == Dc, (name, ref._dc(d["vxl_ijk_list"]))      # the drop-ins take the row width from the lists
    return d, D_cube, Dc


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (list, tuple)):
        for y in x:
            _freeze(y)
    elif isinstance(x, dict):
        for y in x.values():
            _freeze(y)
    return x


@functools.lru_cache(maxsize=None)
def case(name):
    """One case of the table: lists `d`, D_cube, Dc, the denoise masks and the restatement's denoise and adapthresh results, computed once for
    the CPU and the GPU tests alike and read-only from then on."""
    d, D_cube, Dc = build(name)
    masks = denoise_masks(d)
    c = dict(name=name, d=d, D_cube=D_cube, Dc=Dc, masks=masks, dn_ref=ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], masks, D_cube),
             at_ref=ref.adapthresh_ref(*at_args(d, D_cube)))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def many_cubes():
    """577 cubes of Dc = 27, more than the 512 workgroups the global-parent denoise kernel launches: every workgroup serves a second cube, and
    a cube that is not in the map (an emptied mask below and above index 512, an ijk repeated by a later cube) makes it return early on either
    trip. -> dict(d, D_cube, masks, emptied, repeated)"""
    Dc, lattice = 27, (9, 8, 8)
    d = synthetic.sparse_surface(lattice, Dc, thickness=3, amplitude=6.0, seed=11)
    masks = [(np.asarray(p) >= DENOISE_PROB) & (np.asarray(v) >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    full = [c for c, m in enumerate(masks) if m.sum() > 100]                       # cubes the surface crosses
    low = [c for c in full if c + 512 in full]
    emptied = (low[0], low[1] + 512)                                               # (unmapped, mapped) and (mapped, unmapped) pairs
    for c in emptied:
        masks[c] = np.zeros_like(masks[c])
    rep = low[2]                                                                   # its ijk comes again as the last cube: rep leaves the map
    sub = np.random.RandomState(5).rand(len(masks[rep])) < 0.8
    for k in LIST_KEYS:
        d[k].append(d[k][rep][sub])
    masks.append(masks[rep][sub])
    d["cube_ijk_np"] = np.concatenate([d["cube_ijk_np"], d["cube_ijk_np"][rep:rep + 1]])
    assert ref._dc(d["vxl_ijk_list"]) == Dc
    return _freeze(dict(d=d, D_cube=Dc, Dc=Dc, masks=masks, emptied=emptied, repeated=rep))


@functools.lru_cache(maxsize=None)
def extreme_ijk():
    """Three cubes of Dc = 8 in a row of the lattice's x axis, at x = 0, 1 and 2**32 - 1: cubes 0 and 1 share voxels; cube 2 holds the voxels that
    would coincide with cube 0's if 2**32 - 1 + 1 or 0 - 1 wrapped. The contract is int64 arithmetic: cube 2 is nobody's
    neighbour. `wrapped` is the same scene with the cubes at x = 1, 2, 0, what 32-bit arithmetic would make of it."""
    Dc, h = 8, 4
    rs = np.random.RandomState(17)

    def some(n):
        return np.unique(rs.randint(0, Dc, (n, 3)), axis=0)
    a = some(120)
    from_a_hi = a[a[:, 0] >= h] - [h, 0, 0]                  # cube 1 sees cube 0's upper half (v of 0 == u of 1 + h * (1,0,0))
    from_a_lo = a[a[:, 0] < h] + [h, 0, 0]                   # a cube at x = -1 would see the lower half there
    lists = [a, np.unique(np.concatenate([from_a_hi[::2], some(40)]), axis=0), np.unique(np.concatenate([from_a_lo, some(20)]), axis=0)]
    lists = [l[np.argsort((l[:, 0] * Dc + l[:, 1]) * Dc + l[:, 2])].astype(np.uint8) for l in lists]
    assert a.max() == Dc - 1
    d = dict(vxl_ijk_list=lists, prediction_list=[rs.uniform(0.46, 1.0, len(l)).astype(np.float16) for l in lists],
             rayPooling_votes_list=[np.where(rs.rand(len(l)) < 0.8, 6, 2).astype(np.uint8) for l in lists],
             rgb_list=[np.zeros((len(l), 3), np.uint8) for l in lists],
             cube_ijk_np=np.asarray([[0, 5, 7], [1, 5, 7], [2 ** 32 - 1, 5, 7]], np.uint32))
    masks = [(p >= 0.6) & (v >= 4) for p, v in zip(d["prediction_list"], d["rayPooling_votes_list"])]
    return _freeze(dict(d=d, D_cube=Dc, Dc=Dc, masks=masks, wrapped=np.asarray([[1, 5, 7], [2, 5, 7], [0, 5, 7]], np.uint32)))


# ---- the comparison of the CPU planted-fault tests and the GPU tests --------------------------------------------------------------------------
def packed(r):
    """adapthresh_ref's result in the packed form of adapthresh.adapthresh_lists"""
    cat = lambda lists: np.concatenate([np.asarray(m, bool).reshape(-1) for m in lists]) if len(lists) else np.zeros((0,), bool)
    return dict(init_denoised=cat(r["init_denoised"]), thresh=np.asarray(r["thresh"]), choice=np.asarray(r["choice"]),
                masks=np.stack([cat(m) for m in r["masks"]]), denoised=np.stack([cat(m) for m in r["denoised"]]))


def adapthresh_differences(got, want):
    """names of the packed results that are not np.array_equal (thresh as exact float64): [] when `got` is `want`"""
    bad = [k for k in ("init_denoised", "thresh", "choice", "masks", "denoised")
           if np.asarray(got[k]).shape != np.asarray(want[k]).shape or not np.array_equal(got[k], want[k])]
    if np.asarray(got["thresh"]).dtype != np.float64 and "thresh" not in bad:
        bad.append("thresh")
    return bad


def list_differences(got, want):
    """indices of the cubes whose bool arrays differ: [] when the per-cube lists are equal"""
    if len(got) != len(want):
        return ["length"]
    return [i for i, (a, b) in enumerate(zip(got, want)) if np.asarray(a).dtype != bool or np.asarray(a).shape != np.asarray(b).shape
            or not np.array_equal(a, b)]
