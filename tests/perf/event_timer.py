"""The one timing loop of the benches in this directory."""
import torch


def event_time(fn, iters, warmup):
    """Seconds per call of `fn`: `warmup` untimed calls, then `iters` calls between two events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3
