"""The mesh renderer's contract (include/surfacenet_hip.h sn_mesh_render) restated in numpy: the executable form of
the nine rules and of the colour gather. The restatement starts where rule 1 ends: it takes the projected (h, w, z) of every (view, vertex) -
on the GPU tests what sn_project_points returned for the same inputs, on the CPU tests project() below - so it needs no FMA emulation. All
float arithmetic is numpy's float64, which does not contract; everything else is int64.

    render(h, w, z, faces, H, W, near, tol)      -> depth, face, face_pixels, vert_visible, counts (+ cover: covering triangles per pixel)
    colours(h, w, z, vert_visible, images)       -> vert_views, vert_rgb, counts
    project(P, verts)                            -> h, w, z in plain numpy (CPU tests only)
    PLANTS                                       a fault per rule, for tests/test_meshrender_cpu.py
"""
import numpy as np

SUB = 256
GUARD = 1 << 25
SMALL_BOX = 256                                                 # csrc/meshrender_rules.h MRD_SMALL_BOX: the box size that separates the two raster paths
COUNTS = ("n_triangles", "n_clipped", "n_degenerate", "n_rasterised", "n_pairs", "n_pixels", "n_visible", "reserved")
KEYS = ("depth", "face", "face_pixels", "vert_visible", "counts")
PLANTS = ("own_flip", "affine", "tie_last", "floor_snap", "swap", "quad_id", "bracket")


def triangles(faces):
    """(F,3) as it is; (F,4): (a,b,c), (a,c,d) of every quad, in that order: triangle 2 f + half."""
    f = np.asarray(faces, np.int64)
    if f.shape[1] == 3:
        return f
    return np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def project(P, verts):
    """camera.perspectiveProj without rounding, in plain numpy: P (V,3,4), verts (n,3) -> h, w, z each (V,n)."""
    P = np.asarray(P, np.float64)
    x = np.concatenate([np.asarray(verts, np.float64), np.ones((len(verts), 1))], axis=1)
    with np.errstate(all="ignore"):
        q = np.einsum("vij,nj->vin", P, x)
        return q[:, 1] / q[:, 2], q[:, 0] / q[:, 2], q[:, 2].copy()


def snap(h, w, z, near, plant=None):
    """rule 2 for one view -> X, Y int64 (0 where not ok), ok."""
    rnd = np.floor if plant == "floor_snap" else np.rint
    with np.errstate(all="ignore"):
        x, y = rnd(w * 256.0), rnd(h * 256.0)
        ok = np.isfinite(h) & np.isfinite(w) & np.isfinite(z) & (z > near) & (np.abs(x) < GUARD) & (np.abs(y) < GUARD)
    return np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64), ok


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def render_view(h, w, z, tri, nv, n_faces, H, W, near, tol, plant=None):
    X, Y, ok = snap(h, w, z, near, plant)
    depth = np.full((H, W), np.inf)
    win = np.full((H, W), -1, np.int64)
    cover = np.zeros((H, W), np.int32)
    n_clip = n_deg = n_pairs = 0
    for t, c in enumerate(tri.tolist()):
        if not (ok[c[0]] and ok[c[1]] and ok[c[2]]):
            n_clip += 1
            continue
        x, y = [int(X[i]) for i in c], [int(Y[i]) for i in c]
        zc = [float(z[i]) for i in c]
        A2 = _edge(x[1], y[1], x[2], y[2], x[0], y[0])
        if A2 == 0:
            n_deg += 1
            continue
        s = 1 if A2 > 0 else -1
        if plant == "swap" and s < 0:                           # the fault: corners exchanged in the place of the negation
            x, y, zc, s, A2 = [x[0], x[2], x[1]], [y[0], y[2], y[1]], [zc[0], zc[2], zc[1]], 1, -A2
        j0, j1 = max(0, -(-min(x) // SUB)), min(W - 1, max(x) // SUB)
        i0, i1 = max(0, -(-min(y) // SUB)), min(H - 1, max(y) // SUB)
        if j0 > j1 or i0 > i1:
            continue
        px = (SUB * np.arange(j0, j1 + 1, dtype=np.int64))[None, :]
        py = (SUB * np.arange(i0, i1 + 1, dtype=np.int64))[:, None]
        E, inside = [], True
        for k in range(3):
            p, n = (k + 1) % 3, (k + 2) % 3
            e = s * _edge(x[p], y[p], x[n], y[n], px, py)
            dx, dy = s * (x[n] - x[p]), s * (y[n] - y[p])
            owns = dy > 0 or (dy == 0 and dx > 0)
            if plant == "own_flip":
                owns = not owns
            inside = inside & ((e > 0) | ((e == 0) & owns))
            E.append(e)
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            if plant == "affine":
                zp = ((E[0].astype(np.float64) * zc[0] + E[1].astype(np.float64) * zc[1]) + E[2].astype(np.float64) * zc[2]) / float(s * A2)
            else:
                r = [1.0 / v for v in zc]
                S = (E[0].astype(np.float64) * r[0] + E[1].astype(np.float64) * r[1]) + E[2].astype(np.float64) * r[2]
                zp = float(s * A2) / S
        n_pairs += int(inside.sum())
        cover[i0:i1 + 1, j0:j1 + 1] += inside
        d, wn = depth[i0:i1 + 1, j0:j1 + 1], win[i0:i1 + 1, j0:j1 + 1]
        better = inside & ((zp <= d) if plant == "tie_last" else (zp < d))      # ascending t: a tie stays with the smaller index
        d[better] = zp[better]
        wn[better] = t
    hit = win >= 0
    face = np.where(hit, win if (nv == 3 or plant == "quad_id") else win >> 1, -1).astype(np.int32)
    out_depth = np.where(hit, depth, 0.0)
    face_pixels = np.bincount(face[hit], minlength=n_faces)[:n_faces].astype(np.int32) if plant != "quad_id" else np.zeros((n_faces,), np.int32)
    # rule 8
    with np.errstate(all="ignore"):
        front = np.isfinite(h) & np.isfinite(w) & np.isfinite(z) & (z > near) & (np.abs(h) < GUARD) & (np.abs(w) < GUARD)
        hh, ww = np.where(front, h, 0.0), np.where(front, w, 0.0)
        ri, rj = np.rint(hh), np.rint(ww)
        front &= (ri >= 0) & (ri <= H - 1) & (rj >= 0) & (rj <= W - 1)
        fi, fj = np.floor(hh).astype(np.int64), np.floor(ww).astype(np.int64)
    opened = np.zeros(h.shape, bool)
    far = np.zeros(h.shape)
    for di in (0, 1):
        for dj in (0, 1):
            i, j = fi + di, fj + dj
            inside = (i >= 0) & (i < H) & (j >= 0) & (j < W)
            ic, jc = np.clip(i, 0, H - 1), np.clip(j, 0, W - 1)
            full = inside & hit[ic, jc]
            opened |= ~full
            far = np.maximum(far, np.where(full, out_depth[ic, jc], 0.0))
    if plant == "bracket":
        opened[:] = False
    with np.errstate(all="ignore"):
        vis = front & (opened | (z - tol <= far))
    counts = np.asarray([len(tri), n_clip, n_deg, len(tri) - n_clip - n_deg, n_pairs, int(hit.sum()), int(vis.sum()), 0], np.int64)
    return out_depth, face, face_pixels, vis.astype(np.uint8), counts, cover


def render(h, w, z, faces, H, W, near=0.0, tol=0.0, plant=None):
    """h, w, z (V,n_verts) float64, faces (F,3) or (F,4) -> dict of depth (V,H,W) float64, face (V,H,W) int32, face_pixels (V,F) int32,
    vert_visible (V,n_verts) uint8, counts (8,) int64, cover (V,H,W) int32."""
    h, w, z = (np.asarray(a, np.float64) for a in (h, w, z))
    f = np.asarray(faces)
    tri = triangles(f)
    V = h.shape[0]
    views = [render_view(h[v], w[v], z[v], tri, f.shape[1], f.shape[0], H, W, float(near), float(tol), plant) for v in range(V)]
    res = {k: np.stack([r[i] for r in views]) for i, k in ((0, "depth"), (1, "face"), (2, "face_pixels"), (3, "vert_visible"), (5, "cover"))}
    res["counts"] = np.sum([r[4] for r in views], axis=0).astype(np.int64)
    return res


def colours(h, w, z, vert_visible, images):
    """images (V,H,W,3) uint8 -> dict of vert_views (n,) int32, vert_rgb (n,3) uint8, counts (2,) int64."""
    img = np.asarray(images, np.uint8)
    V, H, W = img.shape[:3]
    n = h.shape[1]
    views, total = np.zeros((n,), np.int64), np.zeros((n, 3), np.int64)
    for v in range(V):
        with np.errstate(all="ignore"):
            ok = (np.asarray(vert_visible)[v] != 0) & np.isfinite(h[v]) & np.isfinite(w[v]) & np.isfinite(z[v])
            i, j = np.rint(np.where(ok, h[v], 0.0)), np.rint(np.where(ok, w[v], 0.0))
            ok &= (i >= 0) & (i <= H - 1) & (j >= 0) & (j <= W - 1)
        i, j = np.where(ok, i, 0).astype(np.int64), np.where(ok, j, 0).astype(np.int64)
        views += ok
        total += np.where(ok[:, None], img[v][i, j].astype(np.int64), 0)
    rgb = np.where(views[:, None] > 0, (2 * total + views[:, None]) // np.maximum(2 * views[:, None], 1), 0).astype(np.uint8)
    return dict(vert_views=views.astype(np.int32), vert_rgb=rgb, counts=np.asarray([int((views > 0).sum()), int(views.sum())], np.int64))


def same_bytes(got, want, keys=KEYS):
    """The keys whose bytes differ."""
    return [k for k in keys if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes() or np.asarray(got[k]).shape != np.asarray(want[k]).shape]


# ---- the cases both test files share -----------------------------------------------------------------------------------------------------------
K_CAM = np.asarray([[100.0, 0, 48], [0, 100, 32], [0, 0, 1]])
CAM = K_CAM @ np.asarray([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]])      # K [I | (0,0,5)]: image 64 x 96
CAM_MIRROR = K_CAM @ np.asarray([[-1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]])      # det P[:, :3] < 0
CAM_BEHIND = K_CAM @ np.asarray([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -5]])      # the object behind the camera: everything clipped
AFFINE = np.asarray([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])             # w = x, h = y, z = 1
SPHERE_HW = (64, 96)


def sphere(stacks, slices=None):
    """A UV sphere of radius 1 about the origin, its poles on the z axis, outward triangles: 2 + (stacks - 1) slices vertices, 2 slices
    (stacks - 1) triangles. -> verts (n,3) float64, faces (F,3) int32."""
    slices = 2 * stacks if slices is None else slices
    v = [(0.0, 0.0, 1.0)]
    for k in range(1, stacks):
        th = np.pi * k / stacks
        for j in range(slices):
            ph = 2 * np.pi * j / slices
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda k, j: 1 + (k - 1) * slices + j % slices
    f = []
    for j in range(slices):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for k in range(1, stacks - 1):
        for j in range(slices):
            a, b, c, d = ring(k, j), ring(k + 1, j), ring(k + 1, j + 1), ring(k, j + 1)
            f += [(a, b, c), (a, c, d)]
    last = len(v) - 1
    for j in range(slices):
        f.append((last, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


def grid(quads=False, reverse=False):
    """6 x 6 squares with vertices at (2 i + 1, 2 j + 1, 0), every pixel centre of the block on an edge or a vertex, cut along alternating
    diagonals (or left as quads). Under AFFINE, image 16 x 16."""
    n = 7
    v = np.asarray([(2 * i + 1, 2 * j + 1, 0.0) for j in range(n) for i in range(n)], np.float64)      # vertex j * 7 + i at x = 2 i + 1, y = 2 j + 1
    f = []
    for j in range(6):
        for i in range(6):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            if quads:
                f.append((a, b, c, d))
            elif (i + j) % 2 == 0:
                f += [(a, b, c), (a, c, d)]
            else:
                f += [(a, b, d), (b, c, d)]
    f = np.asarray(f, np.int32)
    return v, np.ascontiguousarray(f[:, ::-1]) if reverse else f


# ---- the named GPU cases (tests/test_gpu_meshrender.py): each -> (P (V,3,4), verts, faces, (H, W), near, tol) ---------------------------------------
PINHOLE = np.asarray([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])           # w = X / Z, h = Y / Z, z = Z: a vertex (w z, h z, z) lands on (h, w)
GRID_CAM = np.asarray([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.1, 1]])        # AFFINE on the plane Z = 0, perspective off it


def at(hwz):
    """(n,3) rows of (h, w, z) -> the world vertices that PINHOLE sends there (up to rounding: the tests feed the restatement the GPU's own
    projection)."""
    a = np.asarray(hwz, np.float64).reshape(-1, 3)
    return np.stack([a[:, 1] * a[:, 2], a[:, 0] * a[:, 2], a[:, 2]], axis=1)


def _soup(tris):
    """(T,3,3) corners (h, w, z) -> verts, faces of T separate triangles."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    return at(t.reshape(-1, 3)), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


def case_sphere12():
    v, f = sphere(12)
    return np.stack([CAM, CAM_MIRROR, CAM_BEHIND]), v, f, SPHERE_HW, 0.0, 0.0


def case_grid(quads):
    """The grid as triangles or as quads, plus (quads) one non-planar quad beside it."""
    v, f = grid(quads)
    if quads:
        n = len(v)
        v = np.concatenate([v, [(13.6, 1.7, -2.0), (15.4, 2.2, 3.0), (15.1, 12.6, -1.0), (13.9, 11.8, 4.0)]])
        f = np.concatenate([f, [[n, n + 1, n + 2, n + 3]]]).astype(np.int32)
    return GRID_CAM[None], v, f, (16, 16), 0.0, 0.0


def case_ties():
    """Two coplanar copies of one triangle at faces 1 and 3 (the smaller wins), and faces 0 and 2 that meet in equal depth along the
    column w = 6 of pixel centres: face 2's corners lie at z = 1/2, 2 and 1, whose reciprocals are exact, so the tie is one of bits."""
    v = np.asarray([(2, 1, 0), (11, 1, 0), (2, 13, 0), (1, 1, -5), (2.5, 1, -5), (1, 3.25, -5), (1, 1, -5), (16, 1, 10), (6, 14, 0)], np.float64)
    f = np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8], [3, 4, 5], [5, 3, 4]], np.int32)
    return GRID_CAM[None], v, f, (16, 16), 0.0, 0.0


def case_big_and_small():
    """Face 0 covers the whole image from far outside it, inside the guard band, behind everything; 2,000 sub-pixel triangles; triangles of
    50 to 5,000 pixels whose boxes lie below, at and above SMALL_BOX; one past the guard band, one with a corner at z = near, one collinear
    after the snap, and a NaN at an unreferenced vertex."""
    H, W, near = 96, 128, 0.5
    rng = np.random.default_rng(7)
    tris = [[(-50000.0, -50000.0, 10.0), (-50000.0, 100000.0, 10.0), (100000.0, -50000.0, 10.0)]]
    c = np.stack([rng.uniform(0, H, 2000), rng.uniform(0, W, 2000), rng.uniform(1, 2, 2000)], axis=1)
    small = c[:, None, :] + np.concatenate([rng.uniform(-0.6, 0.6, (2000, 3, 2)), np.zeros((2000, 3, 1))], axis=2)
    tris += small.tolist()
    box = lambda h0, w0, dh, dw, z: [(h0, w0, z), (h0 + dh, w0, z + 0.25), (h0, w0 + dw, z + 0.5)]      # a box of (dh + 1) x (dw + 1) pixel centres
    tris += [box(3.0, 4.0, 14.0, 15.0, 3.0), box(20.0, 4.0, 15.0, 15.0, 3.0), box(40.0, 4.0, 16.0, 15.0, 3.0),      # 240, 256, 272
             box(60.0, 4.0, 4.0, 9.0, 3.0), box(10.0, 30.0, 69.0, 71.0, 4.0), box(5.0, 100.0, 85.0, 20.0, 5.0)]      # 50, 5,040, 1,806
    tris += [[(5.0, 5.0, 1.0), (9.0, 140000.0, 1.0), (30.0, 5.0, 1.0)],          # a corner past the guard band: clipped
             [(50.0, 50.0, 1.0), (60.0, 50.0, near), (50.0, 60.0, 1.0)],         # a corner at z = near: clipped
             [(10.0, 10.0, 1.0), (10.001, 20.0, 1.0), (10.0, 30.0, 1.0)]]        # collinear after the snap: degenerate
    v, f = _soup(tris)
    v = np.concatenate([v, [(np.nan, 1.0, 1.0)]])               # referenced by no face: allowed
    return PINHOLE[None], v, f, (H, W), near, 0.0


def case_slivers():
    """Long thin triangles: boxes of up to ten thousand pixels, a few pixels covered, several none at all."""
    H, W = 96, 128
    rng = np.random.default_rng(11)
    tris = []
    for k in range(40):
        h0, thick = rng.uniform(2, H - 3), (0.004, 0.05, 0.3, 0.7)[k % 4]
        tris.append([(h0, 2.2 + k % 3, 2.0), (h0 + thick, 125.6 - k % 5, 2.5), (h0 + rng.uniform(-0.2, 0.2), 60.3, 3.0)])      # a box of one or two rows
    for k in range(24):
        a, b, thick = rng.uniform(2, 20), rng.uniform(2, 30), (0.003, 0.08, 0.45)[k % 3]
        tris.append([(a, b, 2.0), (H - 1 - b / 2, W - 1 - a, 4.0), ((a + H - 1 - b / 2) / 2 + thick, (b + W - 1 - a) / 2, 1.5 + k)])      # a diagonal
    v, f = _soup(tris)
    return PINHOLE[None], v, f, (H, W), 0.0, 0.0


def case_borders(shape=(37, 53)):
    """Triangles across each border and each corner of an image that is no multiple of any tile, and two wholly off it."""
    H, W = shape
    tris = []
    for ch, cw in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W / 2), (H - 1, W / 2), (H / 2, 0), (H / 2, W - 1), (H / 2, W / 2)):
        tris.append([(ch - 4.3, cw - 3.1, 2.0), (ch + 5.2, cw - 2.4, 3.0), (ch + 0.4, cw + 6.8, 2.5)])
        tris.append([(ch - 0.3, cw - 0.4, 1.5), (ch + 0.45, cw - 0.2, 1.5), (ch + 0.1, cw + 0.6, 1.6)])
    tris += [[(-9.0, -9.0, 1.0), (-2.0, -8.0, 1.0), (-3.0, -1.0, 1.0)], [(H + 1.0, 3.0, 1.0), (H + 9.0, 4.0, 1.0), (H + 4.0, W + 7.0, 1.0)]]
    v, f = _soup(tris)
    return PINHOLE[None], v, f, (H, W), 0.0, 0.0


def case_off_screen():
    v, f = _soup([[(-9.0, -9.0, 1.0), (-2.0, -8.0, 1.0), (-3.0, -1.0, 1.0)], [(50.0, 3.0, 1.0), (59.0, 4.0, 1.0), (54.0, 70.0, 1.0)]])
    return PINHOLE[None], v, f, (37, 53), 0.0, 0.0


def look_at(verts, shape, axis=2, fill=0.9):
    """A pinhole camera on the positive side of `axis` that looks back along it and holds the finite vertices in about `fill` of the image."""
    v = np.asarray(verts, np.float64)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, ext = (lo + hi) / 2, (hi - lo).max()
    u, r = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.zeros((3, 3))
    R[0, r], R[1, u], R[2, axis] = 1.0, 1.0, -1.0               # image columns along r, rows along u, depth against the axis
    t = -R @ c + np.asarray([0, 0, 3.0 * ext])
    foc = fill * min(shape) * 2.5
    K = np.asarray([[foc, 0, (shape[1] - 1) / 2], [0, foc, (shape[0] - 1) / 2], [0, 0, 1.0]])
    return K @ np.concatenate([R, t[:, None]], axis=1)


def case_many_workgroups():
    """A mesh of 4,600 faces from the orientation stage's table, in two views of 200 x 300."""
    import meshorient_ref as mo
    v, f = mo.CASES["surface_scr"]()
    shape = (200, 300)
    return np.stack([look_at(v, shape, 2), look_at(v, shape, 0)]), np.asarray(v, np.float64), f, shape, 0.0, 0.0


CASES = dict(sphere12=case_sphere12, grid_on_centres=lambda: case_grid(False), grid_quads=lambda: case_grid(True), ties=case_ties,
             big_and_small=case_big_and_small, slivers=case_slivers, borders=case_borders, one_pixel=lambda: case_borders((1, 1)),
             off_screen=case_off_screen, many_workgroups=case_many_workgroups)
