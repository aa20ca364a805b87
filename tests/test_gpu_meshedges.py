"""GPU (-m gpu): the seam between the stages that stand on the mesh edge table (surfacenet_amd/csrc/meshedges.h, sn_meshedges.hip; DESIGN.md
section 4.16). The build is compiled once and every stage starts with the same host sequence in its own workspace, so one context runs the
four stages one after the other on four different meshes - smooth, orient, fill, self-intersections, then the first smooth again - and each
result has to equal, byte for byte, the same call on a context that has run nothing else; the two smoother results equal each other."""
import pytest

import meshfill_ref as fref
import meshintersect_ref as xref
import meshorient_ref as oref
import meshsmooth_ref as sref
from test_gpu_hash_adversary import _bytes

pytestmark = pytest.mark.gpu
ORIGIN, RESOL = (-20.0, -20.0, -20.0), 0.4


def test_one_context_runs_every_stage_as_a_fresh_one_does(gpu_required):
    import surfacenet_amd as sn
    calls = [
        ("smooth", lambda c: c.mesh_smooth(*sref.sphere_case(6, True), 4, origin=ORIGIN, resol=RESOL)),
        ("orient", lambda c: c.mesh_orient(*sref.sheet_case(False), 1, 0, True)),
        ("fill", lambda c: c.mesh_fill(*fref.sphere_hole_case(6), origin=ORIGIN, resol=RESOL)),
        ("intersect", lambda c: c.mesh_intersect(*xref.fold_case())),
    ]
    calls.append(calls[0])
    with sn.Context(cube_D=8, max_samples=1) as ctx:
        shared = [run(ctx) for _, run in calls]
    assert shared[0]["counts"][0] > 0 and shared[2]["counts"][3] == 1 and shared[3]["counts"][3] > 0      # edges, a filled hole, pairs
    for (name, run), got in zip(calls, shared):
        with sn.Context(cube_D=8, max_samples=1) as fresh:
            want = run(fresh)
        if name == "orient":
            assert oref.same_bytes(got, want) == [], name
        elif name == "intersect":
            assert xref.same_bytes(got, want) == [], name
        else:
            assert sorted(got) == sorted(want) and _bytes(got) == _bytes(want), name
    assert _bytes(shared[0]) == _bytes(shared[4])
