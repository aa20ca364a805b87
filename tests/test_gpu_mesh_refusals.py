"""GPU (-m gpu): the mesh stages refuse a bad mesh in the same words (surfacenet_amd/csrc/mesh_input.h, sn_host.h mesh_report_bad; DESIGN.md
section 4.18): Context.mesh_simplify, mesh_smooth and mesh_fill, host form and device form, on the bad-index and bad-coordinate meshes of
tests/mesh_refusals.py, Context.mesh_sample on the bad index. Every entry names the smallest bad face in the same text, also when that face
lies in the second 256-thread workgroup (face 257 of 300), and a good call on the same context afterwards gives the bytes it gave before."""
import numpy as np
import pytest

import mesh_refusals as bad

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4


@pytest.fixture(scope="module")
def ctx(gpu_required):
    from surfacenet_amd import runtime
    return runtime.any_context()


def _stages(ctx):
    return dict(simplify=lambda v, f, device: ctx.mesh_simplify(v, f, 2, 0, origin=ORIGIN, resol=RESOL, device=device),
                smooth=lambda v, f, device: ctx.mesh_smooth(v, f, 2, origin=ORIGIN, resol=RESOL, device=device),
                fill=lambda v, f, device: ctx.mesh_fill(v, f, 64, 1, origin=ORIGIN, resol=RESOL, device=device),
                sample=lambda v, f, device: dict(zip(("points", "tri"), ctx.mesh_sample(v, f, 0.5, device=device))))


def _good(ctx, v, f):
    return {(name, device): {k: a.tobytes() for k, a in run(v, f, device).items()} for name, run in _stages(ctx).items() for device in (False, True)}


@pytest.mark.parametrize("rows,at,later,coord_at", [(4, 2, 5, 3), (51, 257, 280, 257)])
def test_every_entry_names_the_smallest_bad_face_in_the_same_words(ctx, rows, at, later, coord_at):
    from surfacenet_amd import SurfaceNetHipError
    v, f = bad.sheet(rows)
    assert f.shape == (6 * (rows - 1), 3) and v.shape == (4 * rows, 3)
    before = _good(ctx, v, f)
    assert before["fill", False] == before["fill", True] and before["smooth", False] == before["smooth", True]
    cases = [bad.bad_index(v, f, at, later) + (("simplify", "smooth", "fill", "sample"),)]
    for value in (np.nan, 2097144.0):
        cases.append(bad.bad_coordinate(v, f, coord_at, value) + (("simplify", "smooth", "fill"),))
    far, _, text = bad.bad_coordinate(v, f, coord_at, np.nan)       # ... and a bad index at a later face: the smaller face is the one named
    cases.append((far, bad.bad_index(v, f, later, later)[1], text, ("simplify", "smooth", "fill")))
    stages = _stages(ctx)
    for bv, bf, text, names in cases:
        said = set()
        for name in names:
            for device in (False, True):
                with pytest.raises(SurfaceNetHipError) as e:
                    stages[name](bv, bf, device)
                said.add(str(e.value))
        assert len(said) == 1 and text in said.pop(), (text, said)
    assert bad.bad_index(v, f, at, later)[2] == "face %d names a vertex outside [0, %d)" % (at, 4 * rows)
    assert _good(ctx, v, f) == before                          # the context still works, and says what it said
