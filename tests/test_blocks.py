"""The ragged-block layout and the upload helper the device drivers share (kwiiyatta_amd/_blocks.py), on CPU tensors:
no library, no GPU."""
import numpy as np
import pytest
import torch

from kwiiyatta_amd._blocks import Ragged, p, to_device


def old_offsets(lengths):
    """the prefix sum the drivers used to write out"""
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def old_cut(a, o, i, lo=0, hi=0):
    """the slicing lambda of the drivers before the layout class"""
    return a[int(o[i]) + lo:int(o[i + 1]) - hi]


@pytest.mark.parametrize('lengths', [[5, 0, 3, 7], [4], [0], [0, 0, 2], [1] * 6, [], [301, 217, 451]])
def test_offsets(lengths):
    lay = Ragged(lengths)
    want = [0]
    for n in lengths:
        want.append(want[-1] + n)
    assert lay.off == want and lay.off == old_offsets(lengths).tolist()
    assert all(type(o) is int for o in lay.off)
    assert lay.total == sum(lengths) and type(lay.total) is int
    assert len(lay) == len(lengths)


def test_offsets_of_numpy_lengths_are_python_ints():
    lay = Ragged(np.array([3, 0, 2], dtype=np.int64))
    assert lay.off == [0, 3, 3, 5] and all(type(o) is int for o in lay.off)


@pytest.mark.parametrize('shape_tail', [(), (3,)])
@pytest.mark.parametrize('lengths,lo,hi', [([5, 0, 3, 7], 0, 0), ([4], 0, 0), ([0], 0, 0), ([6, 4, 9], 2, 2),
                                           ([6, 4, 9], 1, 0), ([6, 4, 9], 0, 3), ([201, 250], 100, 100)])
def test_views_equal_the_old_cut_and_share_storage(lengths, lo, hi, shape_tail):
    lay = Ragged(lengths)
    width = int(np.prod(shape_tail, dtype=np.int64))
    block = torch.arange(float(lay.total * width)).reshape((lay.total,) + shape_tail)
    off = old_offsets(lengths)
    views = lay.views(block, lo, hi)
    assert len(views) == len(lengths)
    for i, v in enumerate(views):
        want = old_cut(block, off, i, lo, hi)
        assert v.shape == want.shape and torch.equal(v, want)
        assert v.data_ptr() == want.data_ptr() and v.stride() == want.stride()
        assert v.untyped_storage().data_ptr() == block.untyped_storage().data_ptr()       # a view, not a copy
        w = lay.view(block, i, lo, hi)
        assert w.data_ptr() == v.data_ptr() and w.shape == v.shape
    for v in views:                             # writing through a view reaches the block
        v.fill_(-1.0)
    touched = (block == -1.0).reshape(lay.total, width).all(1)
    want_touched = torch.zeros(lay.total, dtype=torch.bool)
    for i in range(len(lengths)):
        want_touched[int(off[i]) + lo:int(off[i + 1]) - hi] = True
    assert torch.equal(touched, want_touched)


@pytest.mark.parametrize('lengths', [[5, 0, 3, 7], [4], [0, 0, 2], [1] * 6])
def test_views_tile_the_block(lengths):
    """lo = hi = 0: every element of the block lies in exactly one view, in order, without gap or overlap"""
    lay = Ragged(lengths)
    block = torch.zeros(lay.total, 2, dtype=torch.float64)
    views = lay.views(block)
    assert [len(v) for v in views] == lengths
    at = block.data_ptr()
    for v in views:                             # each view starts where the one before it ended
        if len(v):
            assert v.data_ptr() == at
        at += v.numel() * v.element_size()
    assert at == block.data_ptr() + block.numel() * block.element_size()
    for v in views:
        v += 1.0
    assert bool((block == 1.0).all())
    assert torch.equal(torch.cat(views), block)


def test_pointer():
    t = torch.arange(6.0)
    assert p(t).value == t.data_ptr() and p(t[2:]).value == t.data_ptr() + 2 * t.element_size()


def test_to_device_on_the_host():
    t = torch.arange(4.0)
    assert to_device(t, 'cpu') is t and to_device(t, None) is t                # a tensor: as it is
    a = np.arange(12.0).reshape(3, 4)[:, ::2]                                   # not contiguous
    for dev in ('cpu', None):
        u = to_device(a, dev)
        assert u.is_contiguous() and u.dtype == torch.float64 and np.array_equal(u.numpy(), a)
    i = np.arange(5, dtype=np.int16)
    assert to_device(i, 'cpu').dtype == torch.int16                             # no coercion unless asked for
    assert to_device(i, 'cpu', dtype=np.float64).dtype == torch.float64
    assert to_device([1.0, 2.0], 'cpu', dtype=np.float64).tolist() == [1.0, 2.0]
