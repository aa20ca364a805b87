"""CPU: the colliding-key cases of tests/hash_adversary.py held to the reference model of linear probing (probe_model), without a GPU.

The late-key condition is a condition on the model, not a measurement of the library: for every builder and every capacity 2^5 .. 2^16 the
case's keys, inserted in list order (a capacity too small for all of them gets the first cap / 2 distinct ones), wrap at least once and walk at
least 3/4 of the late keys inserted (or cap / 2 where that is smaller); at the totals 32 and 512 the cell table is exactly half full. The
coordinate-derived builders are held to the cells their stage's restatement assigns. Three planted faults - a walk that stops at slot `mask`,
a walk cut after 64 steps, a key dropped when its first slot is taken - lose keys of every adversarial case at the capacity its stage uses and
(the cut walk) none of the scenes the suite had; and with the lost keys' entries removed the restatements' results fail the stages' own
comparisons. `pytest -s -k figures` prints the figures profiles/hashadv/README.md records.

Ray pooling's pixel and cell tables and the mesher's brick table have too few candidates for keys late at every capacity: their cases
(hash_adversary.TARGETED) are late at the one capacity the stage's sizing rule gives them, so the rule's constants are read out of the headers,
every case is held to the rule and to the same conditions at that capacity (a wrap, a walk of 64 steps, a key lost to each fault, another
result from the restatement without the lost keys), and the self-intersection grid's case stands with them."""
import os
import re

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


# ---- the cases that are late at the one capacity their stage gives them: ray pooling, the mesher's bricks; and the intersection grid -------------------------
TARGETED = list(ha.TARGETED)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "surfacenet_amd", "csrc")


def _header_constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(found) == 1, (header, name, found)
    return int(found[0])


def test_the_restated_sizing_rules_are_the_kernels():
    """A targeted case is adversarial only while the rule it was built for is the kernel's: the constants are read out of the headers' text."""
    assert ha.RP_LIST == _header_constant("postpass.h", "RP_LIST")
    assert ha.RP_LDS_M == _header_constant("postpass.h", "RP_LDS_M")
    assert ha.RP_LDS_CAP == _header_constant("postpass.h", "RP_LDS_CAP")
    assert ha.MXI_BIG == _header_constant("meshintersect.h", "MXI_BIG")
    assert ha.MXI_OFFSET == _header_constant("meshintersect_rules.h", "MXI_CELL_OFFSET")
    assert ha.LDS_FILL[1] * ha.RP_LDS_M <= ha.LDS_FILL[0] * ha.RP_LDS_CAP < ha.LDS_FILL[1] * (ha.RP_LDS_M + 14)      # 83 %: all but the 5/6 the header promises
    rule = ha.ray_pool_rule
    assert rule(1) == dict(cap=64, lds=True, listed=True) and rule(32)["cap"] == 64 and rule(33)["cap"] == 128
    assert rule(2048)["cap"] == 4096 and rule(2049) == dict(cap=4096, lds=True, listed=True) and rule(3400)["cap"] == 4096
    assert rule(3401) == dict(cap=8192, lds=False, listed=True) and rule(4096)["cap"] == 8192 and rule(4097)["cap"] == 16384
    assert rule(8192) == dict(cap=16384, lds=False, listed=True) and rule(8193) == dict(cap=32768, lds=False, listed=False)
    assert ha.brick_cap(512) == 1024 and ha.intersect_cap(1024) == 16384 and ha.intersect_cap(513) == 16384 and ha.intersect_cap(3, 4) == 1024
    assert np.array_equal(ha.late_at(np.arange(1 << 16), 1024), np.arange(1 << 16)[(ha.mix64(np.arange(1 << 16)) & np.uint64(1023)) >= 1008])


def _model(name, fault=None):
    c, t = ha.targeted(name)
    return ha.probe_model(t["keys"], t["cap"], fault, fill=c.get("fill", (1, 2)))


@pytest.mark.parametrize("name", TARGETED)
def test_targeted_cases_enter_the_keys_their_rule_was_evaluated_for(name):
    c, t = ha.targeted(name)
    keys, cap = t["keys"], t["cap"]
    assert len(keys) == c["rule_n"]                             # the keys entered number what the rule was evaluated for
    at_cap = ha.late_mask(keys, ha.W, cap.bit_length() - 1)
    assert np.array_equal(np.unique(ha.late_at(keys, cap)), np.unique(keys[at_cap]))
    assert np.unique(keys[at_cap]).size >= c["n_late"] and c["n_late"] >= (24 if len(keys) == 32 else 64)
    if name in ha.RAY_POOL:
        m = int((c["pred"].astype(np.float16) > np.float16(c["thresh"])).sum())
        assert m == c["rule_n"] == len(c["selected"]) and c["rule"] == ha.ray_pool_rule(m) and cap == c["rule"]["cap"]
        assert c["rule"]["lds"] == ("_lds" in name) and c["rule"]["listed"] == ("unlisted" not in name)
        assert c["fill"] == (ha.LDS_FILL if c["rule"]["lds"] else (1, 2)) and c["fill"][1] * m <= c["fill"][0] * cap
        views = c["pairs"].reshape(-1).tolist()
        assert len(set(views)) >= 2 and views.count(c["view"]) == 2      # two distinct views at least, the adversarial one repeated
        w, h, d = (x[c["selected"]] for x in ha._project(c["cameras"][c["view"]].tolist(), c["D"]))
        if name.startswith("pixels"):
            assert np.unique(np.stack([w, h], 1), axis=0).shape[0] == m and np.array_equal(ha.pixel_key(w, h), keys)      # one cell per pixel
            assert ((w == -1) & (h == -1)).sum() == 1 and (w < 0).sum() > 10 and (h < 0).sum() > 10 and (np.maximum(w, h) > 5000).any()
            assert int(ha.pixel_key(-1, -1)) ^ 0x8000000080000000 == 0xffffffffffffffff      # (-1, -1) unflipped is the empty sentinel
        else:
            pix = np.unique(np.stack([w, h], 1), axis=0)
            home = (ha.mix64(ha.pixel_key(pix[:, 0], pix[:, 1])) & np.uint64(cap - 1)).astype(np.int64)
            assert 24 <= len(pix) == np.unique(home).size and (pix[:, 0] < 0).any()      # every pixel gets its home slot, whoever comes first
            slot = home[np.searchsorted(pix[:, 0], w)]
            assert np.array_equal(ha.rp_cell_key(slot, d), keys) and np.unique(keys).size == m
            assert np.bincount(np.searchsorted(pix[:, 0], w)).max() > 50      # many cells on one pixel
            p = c["pred"].reshape(-1)[c["selected"]]
            for px in np.unique(w[at_cap]):                     # the late cells hold the largest predictions of their pixels
                assert p[(w == px) & at_cap].min() > p[(w == px) & ~at_cap].max()
            a, b = c["tied"]
            pa, pb = c["pred"].reshape(-1)[[a, b]]
            assert a != b and pa == pb == p.max() and a // c["D"] ** 2 == b // c["D"] ** 2
            alone = ha.rp_votes(c, pairs=[[c["view"], c["view"]]]).reshape(-1)      # the tie goes to the smaller depth bin: view 0 votes for it alone
            near, far = (a, b) if d[c["selected"] == a][0] < d[c["selected"] == b][0] else (b, a)
            assert alone[near] == 2 and alone[far] == 0
    elif name == "bricks_mesh":
        assert c["mask"].all() and c["mask"].size == c["rule_n"] == 512 and cap == ha.brick_cap(c["mask"].size) == c["tables"]["cell"]["cap"] == 1024
        g = nref.world_cells(c["offsets"], c["ijk"], c["cube_ijk"], c["stride_vox"])
        assert np.unique(g, axis=0).shape[0] == 512 and np.array_equal(ha.keys_of_cells((g + 4) >> 2), keys)
        assert c["n_late"] == 384 and at_cap[:384].all() and np.unique(keys[:384]).size == 384 and not at_cap[384:].any()      # one voxel per late brick
        assert not ha.late_mask(keys).sum() > 16                 # late at every capacity: a handful, as the README's "not reached" said
    else:
        import meshintersect_ref as mref
        assert cap == ha.intersect_cap(c["faces"].shape[0]) == 16384 and ha.late_mask(keys).all()      # (these are late at every capacity)
        assert mref.grid_level(c["verts"], c["faces"]) == (0, c["faces"].shape[0])      # the natural level is 0, a triangle in one cell
        cells = np.floor(c["verts"][c["faces"]]).astype(np.int64) + ha.MXI_OFFSET
        assert (cells == c["tri_cell"][:, None, :]).all()       # every corner strictly inside the triangle's late cell
        assert (np.abs(c["verts"] - np.rint(c["verts"])) >= 1.0 / 16).all()
        per_cell = np.unique(keys, return_counts=True)[1]
        assert per_cell.max() == ha.MXI_BIG + 3 and sorted(set(per_cell.tolist())) == [1, 2, ha.MXI_BIG + 3]
        assert _model(name)["walk"][-1] >= 400                   # the big cell is the last key: its slot is the end of the run
        r = mref.intersect(c["verts"], c["faces"])
        assert r["counts"][3] > 200 and r["counts"][2] > r["counts"][3] + 100 and r["counts"][1] == 0      # hits, and candidates that are none
        x8 = ha.intersect_case(8)
        assert np.array_equal(x8["faces"], c["faces"]) and x8["level"] == 3
        cells8 = (np.floor(x8["verts"][x8["faces"]]).astype(np.int64) + ha.MXI_OFFSET) >> 3
        assert (cells8 == c["tri_cell"][:, None, :]).all()      # the same keys at level 3
        assert mref.same_bytes(mref.intersect(x8["verts"], x8["faces"]), r) == []


@pytest.mark.parametrize("name", TARGETED)
def test_targeted_keys_wrap_walk_and_are_lost_to_every_fault(name):
    """The set of occupied slots of linear probing does not depend on the insertion order (a run is filled from its first slot on, whoever comes
    first), and neither does which START slots lie in a run that reaches slot `mask`: that is why this sequential model speaks for the GPU's
    racing inserts. Which key ends where does depend on it, so the conditions count keys and steps; they name no key."""
    c, t = ha.targeted(name)
    m = _model(name)
    n = len(m["keys"])
    assert m["wrapped"].sum() >= 1, name
    if n > ha.LIMIT:
        assert m["walk"].max() >= ha.LIMIT, (name, int(m["walk"].max()))
    for fault in ha.FAULTS:
        lost = len(_model(name, fault)["lost"])
        if fault == "limit" and n <= ha.LIMIT:
            assert lost == 0                                     # 32 keys cannot walk 64 steps
        else:
            assert lost >= 1, (name, fault)
    taken = np.zeros(t["cap"], bool)
    taken[m["slot"]] = True
    again = ha.probe_model(t["keys"][np.random.RandomState(5).permutation(len(t["keys"]))], t["cap"], fill=c.get("fill", (1, 2)))
    other = np.zeros(t["cap"], bool)
    other[again["slot"]] = True
    assert np.array_equal(taken, other) and again["wrapped"].sum() >= 1      # another order: the same slots


@pytest.mark.parametrize("fault", ha.FAULTS)
@pytest.mark.parametrize("name", ha.RAY_POOL)
def test_ray_pooling_notices_lost_keys(name, fault):
    if fault == "limit" and name.endswith("32"):
        return                                                   # (no key to lose)
    c, _ = ha.targeted(name)
    lost = _model(name, fault)["lost"]
    broken = ha.without_voxels(c, lost)
    assert 0 < (broken != c["pred"]).sum() == len(lost)
    assert not np.array_equal(ha.rp_votes(c, broken), ha.rp_want(name))


def test_the_zero_predictions_case_reaches_the_coherent_probe_of_the_lds_tables():
    """ray_pool_kernel calls lt_find<LtKeys, true> for a voxel that stores a 0 on a pixel whose cells all store 0, at another bin than the view's
    minimum: only without a threshold, so with every voxel selected, so in LDS only for a cube of at most 12^3 (the library takes multiples of 4):
    1,728 keys in 4,096 slots. No fault can lose 64 steps there; the case is held to what its camera was searched for: the looked-up key of an
    all-zero slice starts in the last sixteen slots, in a run that passes slot `mask` in any order of the inserts."""
    c, t = ha.targeted("zeros_lds")
    D, m = c["D"], c["D"] ** 3
    assert c["thresh"] is None and m == c["rule_n"] == len(t["keys"]) == np.unique(t["keys"]).size and (D + 4) ** 3 > ha.RP_LDS_M >= m
    assert c["rule"] == ha.ray_pool_rule(m) == dict(cap=4096, lds=True, listed=True)
    w, h, d = ha._project(c["cameras"][0].tolist(), D)
    i = np.arange(m) // (D * D)
    pix = np.unique(np.stack([w, h], 1), axis=0)
    home = (ha.mix64(ha.pixel_key(pix[:, 0], pix[:, 1])) & np.uint64(t["cap"] - 1)).astype(np.int64)
    assert len(pix) == D == np.unique(home).size and np.array_equal(pix[i, 0], w)      # a pixel per i, each at its home slot
    assert np.array_equal(ha.rp_cell_key(home[i], d), t["keys"]) and d.min() == c["dmin"]
    pred = c["pred"].reshape(D, D * D)
    zero = np.nonzero((pred == 0).all(axis=1))[0]
    assert np.array_equal(zero, c["zero_pixels"]) and len(zero) == 3 and 0 not in zero and pred[0, 0] == 0
    assert (d.reshape(D, -1)[:, 0] == c["dmin"]).all()          # every pixel has its cell at the minimum bin: voxel (i, 0, 0)
    lookups = ha.rp_cell_key(home[c["late_pixels"]], c["dmin"])  # the key 143 voxels of a late zero slice each look up
    assert len(lookups) >= 1 and np.isin(c["late_pixels"], zero).all() and np.isin(lookups, t["keys"]).all()
    assert c["n_late"] == 19 == len(ha.late_at(t["keys"], t["cap"])) and np.isin(lookups, ha.late_at(t["keys"], t["cap"])).all()
    model = ha.probe_model(t["keys"], t["cap"])
    taken = np.zeros(t["cap"], bool)
    taken[model["slot"]] = True
    start = int(ha.mix64(lookups).min() & np.uint64(t["cap"] - 1))
    assert start >= t["cap"] - 16 and taken[start:].all() and taken[:8].all()      # the run those lookups start in passes slot `mask` by 8 slots
    assert model["wrapped"].sum() >= 1 and len(ha.probe_model(t["keys"], t["cap"], "no_wrap")["lost"]) >= 1
    alone = ha.rp_votes(c, pairs=[[0, 0]]).reshape(D, D * D)
    assert (alone[zero, 0] == 2).all() and not alone[zero, 1:].any() and alone[0, 0] == 0      # found: the cell votes; missed: voxel 0 would get the vote
    assert (alone > 0).sum() == D


def _fullest_inputs(m):
    """test_gpu_post.test_ray_pool_tables_at_their_fullest's inputs, restated: -> per distinct view the pixel keys and, with the pixel slots the
    model gives in flat order, the cell keys of the selected voxels."""
    from oracle import post_oracle
    import test_gpu_post
    D = 16
    rs = np.random.RandomState(m)
    pred = np.full(D ** 3, 0.1, np.float32)
    pred[rs.permutation(D ** 3)[:m]] = (0.6 + 0.3 * rs.rand(m)).astype(np.float32)
    sel = np.nonzero(pred.astype(np.float16) > np.float16(0.5))[0]
    assert len(sel) == m
    xyz, r = np.asarray([-3.0, 2.0, 640.0], np.float32).astype(np.float64), float(np.float32(0.4))
    i, j, k = np.unravel_index(sel, (D, D, D))
    X, Y, Z = i * r + xyz[0], j * r + xyz[1], k * r + xyz[2]
    cap, fill = ha.ray_pool_rule(m)["cap"], (ha.LDS_FILL if ha.ray_pool_rule(m)["lds"] else (1, 2))
    out = []
    for view in (0, 1, 2):
        q = post_oracle._numerators(test_gpu_post.P_DTU[view], X, Y, Z)
        w, h, d = np.rint(q[0] / q[2]).astype(np.int64), np.rint(q[1] / q[2]).astype(np.int64), np.rint(q[2] / r).astype(np.int64)
        pk = ha.pixel_key(w, h)
        pm = ha.probe_model(pk, cap, fill=fill)
        slot = dict(zip(pm["keys"].tolist(), pm["slot"].tolist()))
        out.append((pk, ha.rp_cell_key([slot[x] for x in pk.tolist()], d), cap, fill))
    return out


@pytest.mark.parametrize("m", [32, 2048, 3400, 4096])
def test_the_fullest_ray_pool_inputs_lose_nothing_to_a_walk_that_stops(m):
    """The seeded voxels under the DTU cameras hash uniformly: in every view's PIXEL table (its keys are the input's own, whatever the order) no
    walk wraps and none is longer than 8 slots, so a walk that stops at slot `mask` or after 64 steps loses none of them. The CELL keys hold the
    pixel's slot, which the race decides; with the slots the model gives in flat order they wrap 0 to 7 keys per view by chance, and at
    m = 3,400 (83 % full) the longest walks are 119, 168 and 65 slots: figures, not conditions, since another order gives other keys. No such
    walk is there by construction."""
    for pk, ck, cap, fill in _fullest_inputs(m):
        model = ha.probe_model(pk, cap, fill=fill)
        assert model["wrapped"].sum() == 0 and model["walk"].max() <= 8
        for fault in ("no_wrap", "limit"):
            assert len(ha.probe_model(pk, cap, fault, fill=fill)["lost"]) == 0, (m, fault)
        assert ha.probe_model(ck, cap, fill=fill)["wrapped"].sum() <= 7      # (this order's; see above)


@pytest.mark.parametrize("fault", ha.FAULTS)
def test_the_intersection_stage_notices_lost_grid_cells(fault):
    import meshintersect_ref as mref
    c, _ = ha.targeted("intersect")
    faces = ha.without_grid_cells(c, _model("intersect", fault)["lost"])
    assert 0 < faces.shape[0] < c["faces"].shape[0]
    want = mref.intersect(c["verts"], c["faces"])
    broken = mref.intersect(c["verts"], faces)
    assert broken["counts"][3] < want["counts"][3] and broken["counts"][4] < want["counts"][4]      # pairs and hit faces go with the cells


@pytest.mark.parametrize("fault", ha.FAULTS)
def test_the_mesher_notices_lost_bricks(fault):
    import mesh_ref as mr
    import test_gpu_mesh
    c, _ = ha.targeted("bricks_mesh")
    broken = ha.without_bricks(c, _model("bricks_mesh", fault)["lost"])
    assert 0 < broken["mask"].sum() < c["mask"].sum()
    want = mr.mesh_ref(*mr.scene_args(c), radius=2, reach=0)
    assert want["quads"].shape[0] > 0 and want["n_cells"] == 512
    with pytest.raises(AssertionError):
        test_gpu_mesh._compare(_mesh_outputs(mr.mesh_ref(*mr.scene_args(broken), radius=2, reach=0)), want)


def _mesh_outputs(r):
    """mesh_ref's dict under the names the stage returns (test_gpu_mesh._compare reads got["verts_lattice"], want["vert_lattice"])."""
    return dict(r, verts_lattice=r["vert_lattice"])


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
    for name in TARGETED + list(ha.FULL):
        c, t = ha.targeted(name)
        m = _model(name)
        at_cap = int(ha.late_mask(m["keys"], ha.W, t["cap"].bit_length() - 1).sum())
        print("| %s | %s | %d | %d | %d | %d, %.0f %% | %d | %d of %d | %d | %d | %d |" % (name, ha.TARGETED.get(name, ha.FULL.get(name))[1], len(t["keys"]), len(m["keys"]), at_cap, t["cap"],
                                                                                            100.0 * len(m["keys"]) / t["cap"], m["walk"].max(), m["wrapped"].sum(), len(m["keys"]),
                                                                                            *[len(_model(name, f)["lost"]) for f in ha.FAULTS]))
    for m_sel in (32, 2048, 3400, 4096):
        for view, (pk, ck, cap, fill) in enumerate(_fullest_inputs(m_sel)):
            for table, keys in (("pixel", pk), ("cell", ck)):
                m = ha.probe_model(keys, cap, fill=fill)
                print("| fullest m = %d, view %d | %s | %d | %d | %d | %d | %d | %d of %d | %d | %d | %d |" % (
                    m_sel, view, table, len(keys), len(m["keys"]), int(ha.late_mask(m["keys"], ha.W, cap.bit_length() - 1).sum()), cap, m["walk"].max(), m["wrapped"].sum(),
                    len(m["keys"]), *[len(ha.probe_model(keys, cap, f, fill=fill)["lost"]) for f in ha.FAULTS]))
    for name, t in _existing().items():
        m = ha.probe_model(t["keys"], t["cap"])
        print("| %s | existing | %d | %d | %d | %d | %d | %d of %d | %d | %d | %d |" % (name, len(t["keys"]), len(m["keys"]), int(ha.late_mask(m["keys"]).sum()), t["cap"],
                                                                                       m["walk"].max(), m["wrapped"].sum(), len(m["keys"]), *[len(_lost(t, f)) for f in ha.FAULTS]))
