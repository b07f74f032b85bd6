"""The inputs of the aperiodicity band codec's edge tests: what the CPU check of the inputs (test_codec_cases.py) and
the GPU test of the kernels (test_codec_edges_gpu.py) share.  The checker is the CPU oracle (ko.code_aperiodicity,
ko.decode_aperiodicity, ko_d4c_num_bands); nothing here imports the product.

Tolerances, derived: the library and the oracle are both built with -ffp-contract=off and evaluate the same
expressions, so they differ only in log10 and pow, by a few ulp.
* code: 20 log10(ap) of ap in [1e-12, 1] lies in [-240, 0] dB, where an ulp is at most 2.9e-14; the interpolation
  adds two such values with weights that sum to 1.  A few ulp of either is below 5e-13: CODE_ABS = 1e-12 dB.
* decode: 10^(v / 20) with the same v on both sides; a few ulp of pow's result is below 1e-15: DECODE_REL = 1e-13."""
import numpy as np

CODE_ABS = 1e-12
DECODE_REL = 1e-13
SAFE = 1e-12                                  # WORLD's kMySafeGuardMinimum
UNVOICED = 1 - SAFE                           # what an unvoiced frame decodes to
INTERVAL = 3000.0                             # band centres at 3 kHz, 6 kHz, ...

RATES = (4000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
BANDS = (0, 0, 0, 1, 1, 2, 3, 4, 5, 5, 5)

# (fs, fft_size): every band count from 1 to 5, transform lengths that are no power of two (what
# _recode_aperiodicity's 2 * (new_spectrum_len - 1) can be), four bins only
PAIRS = ((12000, 512), (16000, 1024), (22050, 1500), (24000, 1024), (32000, 1024), (44100, 2048), (48000, 742),
         (48000, 6), (96000, 4096))
FRAMES = (1, 5)


def bands(fs):
    return BANDS[RATES.index(fs)]


def random_rows(fs, fft_size, T):
    """T rows of 10 ** -U(0.05, 3)"""
    rng = np.random.default_rng([fs, fft_size, T])
    return 10.0 ** -rng.uniform(0.05, 3.0, (T, fft_size // 2 + 1))


def step_bin(fs, fft_size):
    """the bin under the highest band centre"""
    return int(INTERVAL * bands(fs) / (fs / fft_size))


def fixed_rows(fs, fft_size):
    """three rows: all 1 - 1e-12 (coded above -0.5 dB: decodes as unvoiced), all 1e-12 (-240 dB), and a step from 1e-6
    to 0.5 behind the bin under the highest band centre, so that the centre is interpolated across 114 dB"""
    K = fft_size // 2 + 1
    rows = np.empty((3, K))
    rows[0], rows[1] = UNVOICED, SAFE
    k = step_bin(fs, fft_size)
    rows[2, :k + 1], rows[2, k + 1:] = 1e-6, 0.5
    return rows


def inputs(fs, fft_size):
    """name -> (T, K) aperiodicity: the random matrices of 1 and 5 frames and the fixed rows"""
    out = {f'random T={T}': random_rows(fs, fft_size, T) for T in FRAMES}
    out['fixed rows'] = fixed_rows(fs, fft_size)
    return out


# ---- the voicing threshold: coded rows whose sum is exact in binary, (fs, rows, unvoiced flags) --------------------------
def threshold_cases():
    return [(48000, np.array([[-0.5] * 5, [-0.25, -0.75, -0.5, -0.5, -0.5]]), [False, False]),
            (16000, np.array([[np.nextafter(-0.5, 0)], [np.nextafter(-0.5, -1)], [-0.5]]), [True, False, False])]
