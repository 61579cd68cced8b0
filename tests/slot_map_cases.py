"""The sparse frame of the slot-map tests: the eight-model room of path_scenes.py seen
from far off, so most camera rays miss and the survivors of bounce 0 sit in partly
filled and empty compaction chunks.  Test infrastructure: test_slot_map_scene.py holds
the oracle to the condition on the CPU, test_gpu_slot_map.py renders it."""
import path_scenes as S

SPARSE_KEY = ("models", 8)
SPARSE_FRAME = dict(width=64, height=48, iterations=2, max_bounces=5, cam=(0.0, 0.0, 3000.0), plane_z=2980.0)


def sparse_scene(P):
    return S.scene_once(SPARSE_KEY, lambda: S.scene_from_spec(P, *S.model_count_spec(8)))


def sparse_condition(per_bounce, cfg):
    """Fewer than half the pixels live at bounce 1, and bounce 2 not empty
    (per_bounce[b]: rays entering bounce b, summed over the iterations)."""
    launched = cfg.width * cfg.height * cfg.iterations
    assert per_bounce[0] == launched, per_bounce
    assert 0 < per_bounce[1] < launched // 2, per_bounce
    assert per_bounce[2] > 0, per_bounce
