"""Sampling and command-line helpers of the plant-parameter studies (examples/, scripts/bench_plant_params.py, the tests' sampler): not part of the
public interface."""
import numpy as np

from .models import plant_param_defaults, plant_param_names

GIMBAL_LENGTHS = ("gimbal_a", "gimbal_b", "gimbal_c", "gimbal_d", "gimbal_e")


def sample_plant_params(model, seeds, spread_pct=0.0, scale=None):
    """Per-run plant parameters (len(seeds), np) of a robustness study: every parameter of run s drawn uniformly within +-spread_pct % of its default
    from numpy's default_rng(s) -- a function of the run's seed alone, so shards and slices draw the same values -- then `scale` {name: factor}
    applied to every run.  The rocket's gimbal lengths are not spread: the linkage has no real solution far from its design values."""
    names, d = plant_param_names(model), plant_param_defaults(model)
    P = np.tile(d, (len(seeds), 1))
    if spread_pct:
        spread = np.array([0.0 if k in GIMBAL_LENGTHS else 0.01 * float(spread_pct) for k in names])
        for r, s in enumerate(seeds):
            P[r] *= 1.0 + spread * np.random.default_rng(int(s)).uniform(-1.0, 1.0, len(d))
    for k, fct in (scale or {}).items():
        if k not in names:
            raise ValueError(f"sample_plant_params: unknown parameter {k!r} (known: {list(names)})")
        P[:, names.index(k)] *= float(fct)
    return P


def parse_plant_scale(items):
    """["mass=1.15", "servo_angle_time_constant=1.3"] (a command line's repeated --plant-scale NAME=FACTOR) -> {name: factor}."""
    out = {}
    for it in items or []:
        k, sep, v = it.partition("=")
        if not sep:
            raise ValueError(f"--plant-scale takes NAME=FACTOR, got {it!r}")
        out[k.strip()] = float(v)
    return out
