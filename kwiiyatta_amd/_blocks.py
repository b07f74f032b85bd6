"""Plumbing shared by the device drivers (pipeline.py, corpus.py): the data pointer of a tensor, the one way a
caller's array reaches the device, and the layout of a ragged block -- items of different lengths stored end to end in
one contiguous tensor, handed to the batched C entries as per-item views.  Needs neither the library nor a GPU."""
import ctypes
from itertools import accumulate

import numpy as np
import torch


def p(t):
    """the data pointer of a tensor as the `void *` argument of a C entry"""
    return ctypes.c_void_p(t.data_ptr())


def to_device(a, dev, streams=(), dtype=None):
    """A tensor as it is; a numpy array (through `dtype`, if given) as a contiguous tensor on `dev` -- or, with
    dev=None, in host memory still: the source of a `copy_` into a device buffer that exists already.
    streams: the streams besides the current one that will use the result.  They are recorded with the caching
    allocator, which then does not hand the memory out again while their work on it is still queued, whenever the
    caller drops the tensor."""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
        if dev is None:
            return a
        a = a.to(dev)
    for s in streams:
        a.record_stream(s)
    return a


class Ragged:
    """Items of the given lengths end to end along the first axis of a block: item i is
    block[off[i]:off[i + 1]], `total` = off[-1] rows in all."""

    def __init__(self, lengths):
        self.off = list(accumulate((int(n) for n in lengths), initial=0))
        self.total = self.off[-1]

    def __len__(self):
        return len(self.off) - 1

    def view(self, block, i, lo=0, hi=0):
        """item i of `block` without its first `lo` and last `hi` rows"""
        return block[self.off[i] + lo:self.off[i + 1] - hi]

    def views(self, block, lo=0, hi=0):
        return [self.view(block, i, lo, hi) for i in range(len(self))]
