"""What the query bench scripts (raycast_bench.py, raycast_terrain_bench.py, raycast_sensor_bench.py, proximity_bench.py,
contact_sensor_bench.py) share."""
import numpy as np
import torch


def time_calls(call, stream, repeats, warmup=3):
    """(median, min, max) in ms of `repeats` calls of call() after `warmup` untimed ones: HIP events around each call on `stream`, the
    stream a library entry enqueues on; call() returns the entry's status code."""
    ms = []
    for k in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        code = call()
        b.record(stream)
        b.synchronize()
        assert code == 0, code
        if k >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
