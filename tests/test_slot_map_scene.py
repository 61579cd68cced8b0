"""CPU precondition of test_gpu_slot_map.py's sparse case: by the oracle alone, fewer
than half the pixels of slot_map_cases' frame are live at bounce 1 and bounce 2 is
not empty, under both of the oracle's intersections."""
import pytest

from helpers import flat_from_export, oracle_cfg
from slot_map_cases import SPARSE_FRAME, sparse_condition, sparse_scene


@pytest.mark.parametrize("accel", [2, 1], ids=["grid_fast", "bvh"])
def test_sparse_frame_is_sparse(pt_mod, oracle_mod, accel):
    import adaptive_ref as AR
    P = pt_mod
    cfg = P.RenderConfig(accel=accel, **SPARSE_FRAME)
    ref = AR.Restatement(flat_from_export(sparse_scene(P).export()), oracle_cfg(cfg, threads=4))
    ref.render(0, cfg.iterations)
    per = [ref.n_launch * cfg.iterations] + [sum(l[b] for l in ref.live if len(l) > b) for b in range(4)]
    sparse_condition(per, cfg)
    img, seg = oracle_mod.render(ref.flat, oracle_cfg(cfg, threads=4))
    assert seg == ref.segments == sum(sum(l) for l in ref.live) + per[0]      # the restatement is the oracle's loop
