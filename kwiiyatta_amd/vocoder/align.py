"""Time alignment of two feature sets by dynamic time warping.  API of kwiiyatta.vocoder.align
(/root/reference/kwiiyatta/vocoder/align.py): `make_feature` / `dtw_feature` build the DTW features and the warping
path, `align` re-times one feature set onto the other's frames, `align_even` re-times both onto the path.

The warping itself is FastDTW on the GPU (kwiiyatta_amd.backend.dtw, fastdtw's call signature); this module is the
index bookkeeping around it, done with numpy on whole paths.  Observable behaviour follows the reference,
including what its tests and the training path rely on:
  * DTW features are [power term, voicing term, c1 .. cN] of the mel-cepstrum at the lower of the two sampling
    rates; the power term is c0 binarised against a pivot (9.4 above `max(c0) - 1.636` by default);
  * `strict` drops inner path cells whose frames disagree in power class, or whose x-voicing disagrees with the
    y-POWER class -- the second test reads column 0 of y, as the reference does (align.py:78), and defines what
    a strict alignment is;
  * one x per y (`project_path_iter`): the first x of a new y; a jump in y is filled by spreading the x range
    with integer arithmetic; the silence pads are cut off the y axis."""
import numpy as np

from ..backend import dtw as fastdtw


def _pkg():
    import kwiiyatta_amd
    return kwiiyatta_amd


def binalize(x, threshold, ceil, floor=0, out=None):
    """two-level version of x: `ceil` where x >= threshold, `floor` elsewhere"""
    levels = np.where(x >= threshold, ceil, floor)
    if out is None:
        return levels.astype(x.dtype)
    out[...] = levels
    return out


def _power_threshold(c0, pivot, offset):
    if pivot == 'max':
        return c0.max() - offset
    if pivot == 'median':
        return np.median(c0) - offset
    if pivot == 'min':
        return c0.min() + offset
    if pivot == 'fix':
        return offset
    raise ValueError(f'Unknown power_pivot parameter: {pivot!r}')


def make_feature(f, fs, vuv='voiced', vuv_weight=9.0, power='binalize', power_weight=9.4, power_pivot='max',
                 power_threshold=1.636):
    coefficients = f.resample_mel_cepstrum(fs).data
    c0 = coefficients[:, 0]
    rows = np.zeros((len(coefficients), coefficients.shape[1] + 1))
    rows[:, 2:] = coefficients[:, 1:]
    if power == 'binalize':
        binalize(c0, _power_threshold(c0, power_pivot, power_threshold), power_weight, out=rows[:, 0])
    elif power == 'raw':
        rows[:, 0] = c0
    elif power is not None:
        raise ValueError(f'Unknown power parameter: {power!r}')
    if vuv in ('voiced', 'f0'):
        rows[f.is_voiced if vuv == 'voiced' else f.f0 > 0, 1] = vuv_weight
    elif vuv is not None:
        raise ValueError(f'Unknown vuv parameter: {vuv!r}')
    return rows


def dtw_feature(x, y, vuv='voiced', power='binalize', strict=True, radius=32, x_mapped=None, **kwargs):
    """(FastDTW distance, path as an (L, 2) integer array) between the DTW features of x and y.
    x_mapped: a (frames, order) array that takes the place of x's c1..cN in its feature rows (columns 2..) -- x's
    coefficients mapped towards y's speaker, for the re-alignment of a training set; x's power and voicing terms stay
    its own"""
    fs = min(x.fs, y.fs)
    x_rows = make_feature(x, fs, vuv=vuv, power=power, **kwargs)
    if x_mapped is not None:
        x_mapped = np.asarray(x_mapped)
        if x_mapped.shape != x_rows[:, 2:].shape:
            raise ValueError(f'x_mapped is expected to have shape {x_rows[:, 2:].shape} (frames, order) but has '
                             f'{x_mapped.shape}')
        x_rows[:, 2:] = x_mapped
    y_rows = make_feature(y, fs, vuv=vuv, power=power, **kwargs)
    dist, cells = fastdtw.fastdtw(x_rows, y_rows, dist=2, radius=radius)
    path = np.array(cells, dtype=int).reshape(-1, 2)
    if strict:
        # the end cells always stay -- a one-cell path therefore comes out twice, like the reference's chain()
        inner = path[1:-1]
        agree = np.ones(len(inner), dtype=bool)
        y_power = y_rows[inner[:, 1], 0] > 0
        if power == 'binalize':
            agree &= (x_rows[inner[:, 0], 0] > 0) == y_power
        if vuv is not None:
            agree &= (x_rows[inner[:, 0], 1] > 0) == y_power
        path = np.concatenate((path[:1], inner[agree], path[-1:]))
    return dist, path


def project_path_iter(path, trim=True, trim_len=1):
    """one x index per y index of the path: y indices below `trim_len` and the last `trim_len` ones are left out
    when `trim` is set"""
    margin = trim_len if trim else 0
    stop_y = path[-1][1] + 1 - margin          # y indices from here on are not produced
    last_x, last_y = -1, margin - 1
    for x, y in path:
        if y <= last_y:
            continue                           # still the same (or an earlier) y: its x is already out
        if y - last_y == 1:
            if y >= stop_y:
                return
            yield x
        else:                                  # the path skipped y values: ramp x over them
            y = min(y, stop_y - 1)
            steps, rise = y - last_y, x - last_x
            for i in range(steps):
                yield last_x + rise * i // (steps - 1)
        last_x, last_y = x, y


def align(feature, target, vuv='f0', strict=False, pad_silence=True, pad_len=100, **kwargs):
    """`feature` on `target`'s frame axis"""
    if pad_silence:
        pad = _pkg().pad_silence
        feature, target = pad(feature, frame_len=pad_len), pad(target, frame_len=pad_len)
    _, path = dtw_feature(feature, target, vuv=vuv, strict=strict, **kwargs)
    return feature[list(project_path_iter(path, trim=pad_silence, trim_len=pad_len))]


def even_indices(a, b, pad_len=None, **kwargs):
    """the x and y index lists of `align_even` for a and b as they are (padded already, if at all): the warping path
    of `dtw_feature`, cut -- when `pad_len` is given -- to the stretch between the silence pads"""
    _, path = dtw_feature(a, b, **kwargs)
    xs, ys = np.asarray(path).T
    if pad_len is not None:
        # from the first cell inside both signals to the first cell inside both trailing pads; argmax of an
        # all-False mask is 0, which the reference's code shares
        inside = (xs >= pad_len) & (ys >= pad_len)
        beyond = (xs >= a.frame_len - pad_len) & (ys >= b.frame_len - pad_len)
        keep = slice(int(np.argmax(inside)), int(np.argmax(beyond)))
        xs, ys = xs[keep], ys[keep]
    return xs, ys


def align_even(a, b, pad_silence=True, pad_len=100, padded=False, **kwargs):
    """both feature sets along the warping path (same length), without the silence pads.
    padded=True: a and b carry their `pad_len` silent frames already (converter.dataset.PaddedDataset), nothing is
    drawn here.  `x_mapped` (dtw_feature) passes through, as every other option does"""
    if pad_silence and not padded:
        pad = _pkg().pad_silence
        a, b = pad(a, pad_len), pad(b, pad_len)
    xs, ys = even_indices(a, b, pad_len if pad_silence else None, **kwargs)
    return a[xs], b[ys]
