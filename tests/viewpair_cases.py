"""The cases tests/test_viewpair_cpu.py and tests/test_gpu_viewpair.py share: per shape the seeded inputs, the feature rows, the fp64 oracle's weights and the
float32 restatement's (tests/viewpair_check.py), computed once per process and read-only from then on; the synthetic weight lists of both nets."""
import functools

import numpy as np

import viewpair_check as vc
from oracle import net_oracle

SHAPES = vc.SHAPES


@functools.lru_cache(maxsize=None)
def net_values(seed=5):
    from surfacenet_amd import weights
    return weights.synthetic_param_values(seed)


@functools.lru_cache(maxsize=None)
def simil_values(sign=1):
    """weights.synthetic_simil_param_values with the logistic unit of tests/test_gpu_pipeline.py: w = 3, b = -2.5 (sign = -1: both negated)."""
    from surfacenet_amd import weights
    sv = weights.synthetic_simil_param_values(6)
    sv[28][:] = 3.0 * sign; sv[29][:] = -2.5 * sign
    return sv


@functools.lru_cache(maxsize=None)
def case(n_views, n_cubes):
    """One shape's inputs, feature rows, fp64 oracle weights and float32 restatement (MLP values net_values()), computed once for the CPU and the
    GPU tests alike and read-only from then on."""
    c = vc.draw(n_views, n_cubes, seed=100 + n_views)
    c["f"] = vc.features(c["e"], c["d"], c["theta"])
    c["ref"] = net_oracle.relative_weights(c["f"], net_values(), c["P"])
    c["r32"] = vc.restate32_weights(c["f"], net_values(), c["P"])
    c["err32"], c["bound"] = vc.weight_bound(c["r32"], c["ref"])
    c["e_near"] = vc.draw_near(n_views, n_cubes, seed=200 + n_views)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
