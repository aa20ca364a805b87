"""CPU: the colliding-key cases of tests/hash_adversary.py held to the reference model of linear probing (probe_model), without a GPU.

The late-key condition is a condition on the model, not a measurement of the library: for every builder and every capacity 2^5 .. 2^16 the
case's keys, inserted in list order (a capacity too small for all of them gets the first cap / 2 distinct ones), wrap at least once and walk at
least 3/4 of the late keys inserted (or cap / 2 where that is smaller); at the totals 32 and 512 the cell table is exactly half full. The
coordinate-derived builders are held to the cells their stage's restatement assigns. Three planted faults - a walk that stops at slot `mask`,
a walk cut after 64 steps, a key dropped when its first slot is taken - lose keys of every adversarial case at the capacity its stage uses and
(the cut walk) none of the scenes the suite had; and with the lost keys' entries removed the restatements' results fail the stages' own
comparisons. `pytest -s -k figures` prints the figures profiles/hashadv/README.md records."""
import numpy as np
import pytest

import components_ref as cr
import hash_adversary as ha
import meshsimplify_ref as simref
import meshsmooth_ref as smref
import normals_ref as nref
import pointeval_ref
import postpass_cases as cases
import postpass_ref
import ptcubes_ref

CAPS = [1 << c for c in range(5, 17)]
TABLES = [(name, t) for name in ha.BUILDERS for t, _ in ha.tables_of(name)]


def _condition(keys, cap):
    """-> (late keys inserted, longest walk, wrapped insertions, the condition holds) for the first cap / 2 distinct keys of `keys`."""
    m = ha.probe_model(ha.first_distinct(keys, cap // 2), cap)
    n_late = int(ha.late_mask(m["keys"]).sum())
    longest, wrapped = int(m["walk"].max()), int(m["wrapped"].sum())
    return n_late, longest, wrapped, wrapped >= 1 and longest >= min(0.75 * n_late, cap / 2)


# ---- the hash and the figures the key sets were chosen by -----------------------------------------------------------------------------------------------
def test_hashes_are_the_librarys():
    pins = {0x0000040000400003: 0x21d38bd8, 1: 0x34c2cb2c, 0x0123456789abcdef: 0x89022cea, 0x7fffffffffffffff: 0xa930edea}      # tests/host/lattice_check.cpp
    for k, low in pins.items():
        assert int(ha.mix64(np.asarray([k], np.uint64))[0]) & 0xffffffff == low
    assert int(ha.mix64(np.asarray([0], np.uint64))[0]) == 0
    assert int(ha.lt_key(1, 2, 3)) == (1 << 42) | (2 << 21) | 3
    i, j, k = 5, 7, 2 ** 32 - 1                                 # cc_hash in Python integers
    x = ((i * 0x9E3779B97F4A7C15) ^ ((j + 0x632BE59BD9B4E019) * 0xC2B2AE3D27D4EB4F) ^ (k * 0x165667B19E3779F9)) & (2 ** 64 - 1)
    assert int(ha.cc_hash(i, j, k)) == x
    assert ha.table_cap(32, 2, 64) == 64 and ha.table_cap(33, 2, 64) == 128 and ha.table_cap(477, 4, 2048) == 2048 and ha.table_cap(0, 2, 64) == 64


def test_late_cells_of_the_block_in_key_order():
    """475 late cells at w = 4 and 990 at w = 5. In plain key order, for every capacity from 128 slots up, the longest walk is within 6 steps of
    the number inserted and at least 3/4 of the insertions wrap."""
    cells = ha.late_cells()
    assert len(cells) == 475 and len(ha.late_cells(5, 16)) == 990
    keys = ha.keys_of_cells(cells)
    a = np.arange(ha.BLOCK)
    block = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(ha.late_keys(ha.keys_of_cells(block)), keys)      # late_keys of the block's cells under lt_key
    assert ha.late_mask(keys).all() and np.array_equal(np.sort(keys), keys)
    for cap in CAPS[2:]:
        n = min(len(keys), cap // 2)
        m = ha.probe_model(keys[:n], cap)
        assert (m["slot"] >= 0).all() and np.unique(m["slot"]).size == n
        assert n - 6 <= m["walk"].max() <= n and m["wrapped"].sum() >= 0.75 * n, (cap, n, int(m["walk"].max()), int(m["wrapped"].sum()))
        start = (ha.mix64(keys[:n]) & np.uint64(cap - 1)).astype(np.int64)
        assert (start >= cap - 16).all()                        # every walk starts in the last sixteen slots
    assert ha.probe_model(keys, 1024)["walk"].max() == 471 and ha.probe_model(keys, 1024)["wrapped"].sum() == 459


def test_the_model_is_linear_probing():
    """probe_model against the plainest loop, faults included."""
    rs = np.random.RandomState(3)
    keys = np.concatenate([ha.keys_of_cells(ha.late_cells()[:40]), rs.randint(0, 2 ** 40, 60).astype(np.uint64)])
    keys = np.concatenate([keys, keys[::5]])[rs.permutation(120)]
    for cap in (256, 512):
        for fault in (None,) + ha.FAULTS:
            tab, where, lost = [None] * cap, {}, []
            for key in keys.tolist():
                if key in where or key in lost:
                    continue
                h = int(ha.mix64(np.asarray([key], np.uint64))[0]) & (cap - 1)
                steps = 0
                while tab[h] is not None:
                    if (fault == "no_wrap" and h == cap - 1) or (fault == "lost_race"):
                        break
                    h, steps = (h + 1) & (cap - 1), steps + 1
                    if fault == "limit" and steps >= ha.LIMIT:
                        break
                if tab[h] is None:
                    tab[h], where[key] = key, h
                else:
                    lost.append(key)
            m = ha.probe_model(keys, cap, fault)
            assert m["lost"].tolist() == lost and {k: s for k, s in zip(m["keys"].tolist(), m["slot"].tolist()) if s >= 0} == where, (cap, fault)


# ---- the condition ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,table", TABLES, ids=["%s-%s" % t for t in TABLES])
def test_late_keys_wrap_and_walk_at_every_capacity(name, table):
    case = ha.BUILDERS[name]()
    keys = case["tables"][table]["keys"]
    for cap in CAPS:
        n_late, longest, wrapped, ok = _condition(keys, cap)
        assert ok, "%s %s at %d slots: %d late keys, longest walk %d, %d wrapped" % (name, table, cap, n_late, longest, wrapped)
    cap = case["tables"][table]["cap"]
    assert cap <= 1 << 16 and 2 * np.unique(keys).size <= cap   # the stage's own table: at most 2^16 slots, at most half full
    if name in ha.HALF_FULL:
        assert 2 * np.unique(keys).size == cap == 2 * case["mask"].size      # exactly half full
    if name.startswith("edges"):
        assert case["n_late"] >= 256


def test_a_random_sample_of_the_same_size_is_not_adversarial():
    """The condition is about the late keys: 475 cells of the block drawn at random walk a handful of slots at every capacity from 2,048 up."""
    a = np.arange(ha.BLOCK)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    keys = ha.keys_of_cells(g[np.random.RandomState(1).choice(len(g), 475, replace=False)])
    for cap in CAPS[6:]:
        m = ha.probe_model(keys, cap)
        assert m["walk"].max() < 16
        n_late = int(ha.late_mask(keys).sum())
        assert n_late <= 2
    assert not any(ha.probe_model(keys, cap)["walk"].max() >= 0.75 * 475 for cap in CAPS[5:])


# ---- the coordinate-derived builders give the intended cells ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cell", [1, 3])
def test_reduction_grid_cells(per_cell):
    c = ha.reduce_case(per_cell)
    p = c["xyz"]
    h = c["dst"] * (1.0 + 1e-6)                                 # pointeval_ref.neighbour_pairs: cells a little larger than dst, from the min corner
    assert h == c["h"] and np.array_equal(np.floor((p - p.min(axis=0)) / h).astype(np.int64), c["cells"])
    assert np.floor((p.max(axis=0) - p.min(axis=0)) / h).tolist() == [ha.BLOCK - 1] * 3
    keep = pointeval_ref.reduce_rounds(p, c["order"], c["dst"])
    assert keep.all() if per_cell == 1 else 0 < keep.sum() < len(p)


def test_nn_query_grid_cells():
    c = ha.nn_case()
    hq, occ = ha.nn_query_cell(c["to"])
    assert occ == 512 and hq == c["h"]                          # one point per cell at the first bucketing: m0 = 1, h = h0 cbrt(6)
    f = c["frm"]
    assert np.array_equal(np.floor((f - f.min(axis=0)) / hq).astype(np.int64), c["cells"])
    d2 = pointeval_ref.nn_d2(c["to"], f)
    assert np.isfinite(d2).all() and (d2 < 1.0).sum() == 20      # the twenty queries beside `to` points
    # a last-bit difference in the derived cell size (another cbrt) moves no query: every centre is half a cell from its faces
    for scale in (1 - 1e-12, 1 + 1e-12):
        assert np.array_equal(np.floor((f - f.min(axis=0)) / (hq * scale)).astype(np.int64), c["cells"])


def test_gt_grid_cells():
    c = ha.gt_case()
    p = c["pts"]
    assert p.dtype == np.float32
    o = p.min(axis=0).astype(np.float64)                        # cellgrid.h: floor((x - o) / cell) in float64 from the float32 min corner
    assert np.array_equal(np.floor((p.astype(np.float64) - o) / c["cell"]).astype(np.int64), c["cells"])
    import gtcubes_ref
    Y = gtcubes_ref.gt_cubes(p, c["xyz"], c["resol"], c["s"])
    assert (Y.reshape(len(Y), -1).sum(axis=1) >= 1).all() and Y.sum() > 2 * len(Y)
    side = c["s"] * 0.4
    assert (np.floor(side * (1 + 1e-3) / c["cell"]) + 2) ** 3 <= len(p)      # the candidate box holds fewer cells than there are points


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ptcubes_floor_cells(dtype):
    c = ha.ptcubes_case(dtype)
    cubes, _ = ptcubes_ref.quantizePts2Cubes(c["pts"], **ha.PT_ARGS)
    q = c["cells"]
    want = np.unique(np.concatenate([ha.keys_of_cells(q), ha.keys_of_cells(q + 1)]))
    assert np.array_equal(ha.keys_of_cells(cubes["ijk"].astype(np.int64)), want)
    assert (cubes["ijk"].max(axis=0).astype(np.int64) + 1).prod() > 1 << 27      # too many cells for the bitmap form
    assert np.array_equal(np.sort(c["tables"]["set"]["keys"]), np.sort(np.concatenate([ha.keys_of_cells(q), ha.keys_of_cells(q + 1)])))


def test_simplify_cluster_cells_and_face_keys():
    c = ha.simplify_case()
    assert np.array_equal(ha.simplify_cells(c["verts"], c["cell"]), c["cells"])
    r = simref.simplify(c["verts"], c["faces"], c["cell"])
    P = c["n_late"]
    assert r["clusters"] == P and r["vert_cluster"][:P].tolist() == list(range(P))      # cluster k = vertex k: the face keys are the intended ones
    assert np.array_equal(r["vert_cluster"][P:], np.arange(0, P, 4))
    assert r["collapsed"] == len(range(0, P, 4)) and r["duplicates"] == c["n_late_faces"] // 4 and r["largest"] == 2
    assert ha.late_mask(c["tables"]["face"]["keys"][:c["n_late_faces"]]).all()
    assert ha.late_mask(c["tables"]["vertex"]["keys"][:P]).all()
    assert np.array_equal(r["face_src"][:c["n_late_faces"]], np.arange(c["n_late_faces"]))


def test_packed_scenes_enter_the_intended_keys():
    for total, bias in ((32, 0), (512, 0), (1500, 0), (32, 4), (512, 4), (1500, 4)):
        s = ha.cells_case(total, bias)
        g = nref.world_cells(s["offsets"], s["ijk"], s["cube_ijk"], s["stride_vox"])
        n = s["n_late"]
        assert ha.late_mask(ha.keys_of_cells(g[:n] + bias)).all() and g.min() >= 0 and s["normals"].shape == (len(g), 3)
        if total == 1500:
            again = g[s["offsets"][1]:]
            assert len(again) == 2 * len(range(0, n, 4)) and ha.late_mask(ha.keys_of_cells(again + bias)).all()
            assert len(s["cube_ijk"]) >= 4 and 1300 <= len(g) <= 1700 and not s["mask"].all()
    b = ha.bricks_case()
    g = nref.world_cells(b["offsets"], b["ijk"], b["cube_ijk"], b["stride_vox"])
    assert ha.late_mask(ha.keys_of_cells(g[:3 * b["n_late"]] >> 2)).all() and np.unique(g[:3 * b["n_late"]] >> 2, axis=0).shape[0] == b["n_late"]


# ---- the gap is real ------------------------------------------------------------------------------------------------------------------------------------------
def _lost(table, fault):
    return ha.probe_model(table["keys"], table["cap"], fault)["lost"]


@pytest.mark.parametrize("name,table", TABLES, ids=["%s-%s" % t for t in TABLES])
def test_each_fault_loses_keys_of_every_adversarial_case(name, table):
    t = ha.BUILDERS[name]()["tables"][table]
    for fault in ha.FAULTS:
        n = len(_lost(t, fault))
        if fault == "limit" and np.unique(t["keys"]).size <= ha.LIMIT:
            assert n == 0                                        # 32 keys cannot walk 64 steps: the cut walk shows from the 512-voxel cases up
        else:
            assert n >= 1, (name, table, fault)


def _existing():
    out = {"random_cube": ha.scene_keys(cr.random_cube()[0]), "seam_scene(2)": ha.scene_keys(cr.seam_scene(2)), "seam_scene(8)": ha.scene_keys(cr.seam_scene(8))}
    for quads in (True, False):
        out["sphere_case(6) %s" % ("quads" if quads else "triangles")] = ha.mesh_edge_table(smref.sphere_case(6, quads)[1])
    return out


def test_the_existing_scenes_never_walk_far():
    for name, t in _existing().items():
        m = ha.probe_model(t["keys"], t["cap"])
        assert len(_lost(t, "limit")) == 0 and m["walk"].max() < 16, name
        assert len(_lost(t, "no_wrap")) <= 3, name              # a key or two near slot `mask`, by chance


# ---- the stages can tell ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ha.FAULTS)
def test_components_and_unique_voxels_notice_lost_cells(fault):
    s = ha.cells_case(512)
    broken = ha.without_cells(s, _lost(s["tables"]["cell"], fault))
    assert broken["mask"].sum() < s["mask"].sum()
    want = cr.components_ref(*cr.scene_args(s))
    with pytest.raises(AssertionError):
        cr.compare(cr.components_ref(*cr.scene_args(broken)), want)
    keep = nref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], s["mask"], s["stride_vox"])
    assert not np.array_equal(nref.unique_ref(s["offsets"], s["ijk"], s["cube_ijk"], broken["mask"], s["stride_vox"]), keep)
    # the scene with repeats: a lost cell takes all its listings with it
    s = ha.cells_case(1500)
    broken = ha.without_cells(s, _lost(s["tables"]["cell"], fault))
    with pytest.raises(AssertionError):
        cr.compare(cr.components_ref(*cr.scene_args(broken)), cr.components_ref(*cr.scene_args(s)))


@pytest.mark.parametrize("fault", ha.FAULTS)
def test_denoise_notices_lost_cubes(fault):
    c = ha.cubemap_case()
    d = c["d"]
    want = postpass_ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], c["masks"], c["D_cube"])
    assert sum(w.any() for w in want) == len(want) - 1 == 2 * c["n_late"] and not want[c["repeated"]].any()      # every cube but the repeated one keeps voxels
    broken = postpass_ref.denoise_ref(d["cube_ijk_np"], d["vxl_ijk_list"], ha.without_cubes(c, _lost(c["tables"]["map"], fault)), c["D_cube"])
    assert cases.list_differences(broken, want) != []


@pytest.mark.parametrize("nv", [3, 4])
@pytest.mark.parametrize("fault", ha.FAULTS)
def test_the_smoothers_edge_statistics_notice_lost_edges(fault, nv):
    import test_gpu_meshsmooth
    c = ha.edges_case(nv)
    want = smref.smooth(c["verts"], c["faces"], 0)
    assert want["counts"][1] > 100 and want["counts"][2] > 100     # boundary and non-manifold sides among the late ones
    faces = ha.without_edges(c["faces"], _lost(c["tables"]["edge"], fault))
    assert 0 < faces.shape[0] < c["faces"].shape[0]
    with pytest.raises(AssertionError):
        test_gpu_meshsmooth._compare(smref.smooth(c["verts"], faces, 0), want)


# ---- the figures ----------------------------------------------------------------------------------------------------------------------------------------------
def test_figures():
    """What profiles/hashadv/README.md records (run with -s)."""
    print()
    print("| case | table | keys | distinct | late | stage's slots | longest walk there | wrapped there | no_wrap | limit | lost_race |")
    for name, table in TABLES:
        t = ha.BUILDERS[name]()["tables"][table]
        m = ha.probe_model(t["keys"], t["cap"])
        lost = [len(_lost(t, f)) for f in ha.FAULTS]
        print("| %s | %s | %d | %d | %d | %d | %d | %d of %d | %d | %d | %d |" % (name, table, len(t["keys"]), len(m["keys"]), int(ha.late_mask(m["keys"]).sum()),
                                                                                 t["cap"], m["walk"].max(), m["wrapped"].sum(), len(m["keys"]), *lost))
        worst = min((_condition(t["keys"], cap)[1] / max(min(0.75 * _condition(t["keys"], cap)[0], cap / 2), 1), cap) for cap in CAPS)
        assert worst[0] >= 1
    for name, t in _existing().items():
        m = ha.probe_model(t["keys"], t["cap"])
        print("| %s | existing | %d | %d | %d | %d | %d | %d of %d | %d | %d | %d |" % (name, len(t["keys"]), len(m["keys"]), int(ha.late_mask(m["keys"]).sum()), t["cap"],
                                                                                       m["walk"].max(), m["wrapped"].sum(), len(m["keys"]), *[len(_lost(t, f)) for f in ha.FAULTS]))
