"""The timing loop of the tools/*_timing.py programs: blocks of work timed with device events."""
import torch


def block_ms(run_block):
    """ms of one call of run_block, between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run_block()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def blocks(run_block, n_blocks=7, warmup=None):
    """ms of each of n_blocks timed blocks after one warm-up block (or one call of `warmup`), sorted: [n_blocks // 2] is the median."""
    (warmup or run_block)()
    torch.cuda.synchronize()
    return sorted(block_ms(run_block) for _ in range(n_blocks))
