"""The numpy INCA of tests/inca_cases.py on its synthetic set: the monitor falls from fit to fit.  No device."""
import numpy as np
import pytest

import inca_cases


@pytest.mark.parametrize('seed', range(5))
def test_the_monitor_falls_from_fit_to_fit(seed):
    source, target = inca_cases.synthetic(seed)
    xs, ys = np.concatenate(source), np.concatenate(target)
    history, matrices, convert = inca_cases.inca(xs, ys, 4)
    monitor = [r['mcd'] for r in history]
    print(f'seed {seed}: monitor ' + ' -> '.join(f'{v:.3f}' for v in monitor) + ' dB')
    assert all(b < a for a, b in zip(monitor, monitor[1:]))
    assert all(r['rows'] == len(xs) + len(ys) for r in history)
    assert all(m.shape == (len(xs) + len(ys), 2 * inca_cases.ORDER) for m in matrices)
    # the joint rows carry the original source rows, whatever the search looked at
    assert np.array_equal(matrices[-1][:len(xs), :inca_cases.ORDER], xs)
    assert np.array_equal(matrices[-1][len(xs):, inca_cases.ORDER:], ys)
    # the map has learnt the ramp and the gain, roughly: the converted source sits where the target does
    assert abs(convert(xs).mean() - ys.mean()) < 0.1


def test_identical_sides_pair_with_themselves():
    source, _ = inca_cases.synthetic(7)
    xs = np.concatenate(source)
    history, matrices, _ = inca_cases.inca(xs, xs.copy(), 0)
    assert history[0]['mcd'] == 0.0
    assert np.array_equal(matrices[0][:, :inca_cases.ORDER], matrices[0][:, inca_cases.ORDER:])
