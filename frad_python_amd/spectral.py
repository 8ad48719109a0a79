"""``Spectral``: the spectral stage of ``StreamIndex.decode(..., features=spec)`` -- power, magnitude, filterbank and log-mel
spectrograms of the decoded windows, computed on the device by ``frad_clips_spectrum`` (include/frad_hip.h).

The arithmetic, per window ``X`` [rows, K] (float64; what the same call gives without ``features``), rows outside it zero:

* framing: frame f covers rows ``f * hop .. f * hop + n_fft - 1`` (``center=False``) or ``f * hop - n_fft // 2 ..``
  (``center=True``; rows before 0 are zero too: torch's ``pad_mode="constant"``); ``frame_count`` gives F;
* window: ``n_fft`` float64 weights -- ``win_length`` of them ("hann" periodic ``0.5 - 0.5 cos(2 pi n / win_length)``,
  "hamming" ``0.54 - 0.46 cos(..)``, "rect", or an explicit array) centred by ``(n_fft - win_length) // 2`` zeros on the left;
* transform: ``X_f[k] = sum_n x[n] w[n] exp(-2 pi i k n / n_fft)``, k = 0 .. n_fft/2, unnormalised, float64;
* value: ``|X_f[k]|^2`` (``power=2``) or ``|X_f[k]|`` (``power=1``);
* filterbank (optional): ``M[m] = sum_k W[m][k] P[k]`` over the contiguous non-zero band of row m;
* logarithm (optional): ``s * log(max(v, floor))``, s = 1 ("ln"), 1 / ln 10 ("log10"), 10 / ln 10 ("db");
* output: float32 or float64, ``[F, K, n_bins]`` per window: the torch layout ``[K, n_bins, F]`` is ``permute(1, 2, 0)`` of it
  (``[B, K, n_bins, F]`` is ``feature_batch.permute(0, 2, 3, 1)``), a view.

``clips_spectrum_host`` is that definition in numpy (``np.fft.rfft``): the tests' model, and the path of a bridge without the
kernel.  numpy only: nothing here touches the device."""
from __future__ import annotations

import math

import numpy as np

N_FFT = (128, 256, 512, 1024, 2048, 4096)
LOG_SCALE = {"ln": 1.0, "log10": 1.0 / math.log(10.0), "db": 10.0 / math.log(10.0)}


def frame_count(rows: int, n_fft: int, hop: int, center: bool) -> int:
    """frames of a window of ``rows`` rows: ``1 + rows // hop`` centred, else ``1 + (rows - n_fft) // hop`` (0 below n_fft)"""
    if center:
        return 1 + rows // hop
    return 1 + (rows - n_fft) // hop if rows >= n_fft else 0


def hz_to_mel(f, mel: str = "htk"):
    """HTK: ``2595 log10(1 + f / 700)``.  Slaney: ``3 f / 200`` below 1000 Hz, ``15 + 27 ln(f / 1000) / ln 6.4`` above."""
    f = np.asarray(f, np.float64)
    if mel == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f * (3.0 / 200.0), 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / math.log(6.4)))


def mel_to_hz(m, mel: str = "htk"):
    """the inverse of ``hz_to_mel``"""
    m = np.asarray(m, np.float64)
    if mel == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (math.log(6.4) / 27.0)))


def mel_filterbank(srate, n_fft, n_mels, fmin=0.0, fmax=None, mel="htk", norm=None) -> np.ndarray:
    """The triangular mel bank, float64 ``[n_mels, n_fft/2 + 1]``.  ``n_mels + 2`` points equally spaced on the mel scale from
    ``fmin`` to ``fmax`` (default ``srate / 2``) give the edges ``f_0 .. f_{n_mels+1}`` in Hz (``hz_to_mel`` / ``mel_to_hz``:
    HTK ``2595 log10(1 + f/700)``; Slaney linear ``3f/200`` below 1 kHz and logarithmic, step ``ln(6.4)/27``, above).  Row m at
    bin frequency ``f = k * srate / n_fft`` is ``max(0, min((f - f_m) / (f_{m+1} - f_m), (f_{m+2} - f) / (f_{m+2} - f_{m+1})))``;
    ``norm="slaney"`` scales row m by ``2 / (f_{m+2} - f_m)``."""
    if mel not in ("htk", "slaney") or norm not in (None, "slaney"):
        raise ValueError(f"mel is 'htk' or 'slaney' and norm None or 'slaney' (got {mel!r}, {norm!r})")
    if n_mels < 1 or srate < 1:
        raise ValueError(f"n_mels and the sample rate are at least 1 (got {n_mels}, {srate})")
    fmax = srate / 2.0 if fmax is None else float(fmax)
    if not 0.0 <= fmin < fmax <= srate / 2.0:
        raise ValueError(f"the mel bank needs 0 <= fmin < fmax <= srate / 2 (got {fmin}, {fmax}, {srate})")
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin, mel), hz_to_mel(fmax, mel), n_mels + 2), mel)
    f = np.arange(n_fft // 2 + 1) * (srate / n_fft)
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    bank = np.maximum(0.0, np.minimum((f - lo) / (mid - lo), (hi - f) / (hi - mid)))
    if norm == "slaney":
        bank = bank * (2.0 / (hi - lo))
    return bank


def make_window(window, win_length: int, n_fft: int) -> np.ndarray:
    """the ``n_fft`` weights: ``win_length`` named or given ones behind ``(n_fft - win_length) // 2`` zeros"""
    n = np.arange(win_length)
    if isinstance(window, str):
        if window == "hann":
            w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
        elif window == "hamming":
            w = 0.54 - 0.46 * np.cos(2.0 * np.pi * n / win_length)
        elif window == "rect":
            w = np.ones(win_length)
        else:
            raise ValueError(f"window is 'hann', 'hamming', 'rect' or an array of win_length weights (got {window!r})")
    else:
        try:
            w = np.array(window, np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"window is not a float64 array: {e}") from None
        if w.shape != (win_length,):
            raise ValueError(f"window needs win_length = {win_length} weights (got shape {list(w.shape)})")
        if not np.isfinite(w).all():
            raise ValueError("window is not finite")
    full = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    full[left:left + win_length] = w
    return full


def bands_of(bank: np.ndarray):
    """a dense ``[n_bins, n_fft/2 + 1]`` matrix -> (band_lo, band_len, band_off, weights): row m's first to last non-zero entry,
    holes of zeros inside kept as explicit weights; a row of zeros is a band of length 0"""
    lo, ln, off, flat, at = [], [], [], [], 0
    for row in bank:
        nz = np.flatnonzero(row)
        a, b = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        lo.append(a), ln.append(b - a), off.append(at)
        flat.append(row[a:b])
        at += b - a
    w = np.concatenate(flat) if flat else np.zeros(0)
    return np.asarray(lo, np.int32), np.asarray(ln, np.int32), np.asarray(off, np.int64), np.ascontiguousarray(w, np.float64)


class SpecTables:
    """What one ``frad_clips_spectrum`` launch needs besides the windows, on the host: the geometry, the ``n_fft`` window
    weights, the bands (None without a filterbank), the logarithm's constants and the output type.  ``key`` names the tables'
    content for a cache of uploads."""

    def __init__(self, n_fft, hop, center, power, window, bands, log_scale, floor, dtype, key=None):
        self.n_fft, self.hop, self.center, self.power = n_fft, hop, bool(center), power
        self.window = window
        self.band_lo, self.band_len, self.band_off, self.band_w = bands if bands is not None else (None, None, None, None)
        self.log_scale = float(log_scale)
        self.floor = float(floor) if floor is not None else 0.0
        self.floor_log = self.log_scale * math.log(self.floor) if self.log_scale and self.floor > 0 else 0.0
        self.dtype = np.dtype(dtype)
        self.n_bins = len(self.band_lo) if bands is not None else n_fft // 2 + 1
        self.key = key

    def dense_bank(self):
        """the bands as the dense matrix [n_bins, n_fft/2 + 1] (None without a filterbank)"""
        if self.band_lo is None:
            return None
        bank = np.zeros((self.n_bins, self.n_fft // 2 + 1))
        for m in range(self.n_bins):
            a, n, o = int(self.band_lo[m]), int(self.band_len[m]), int(self.band_off[m])
            bank[m, a:a + n] = self.band_w[o:o + n]
        return bank


class Spectral:
    """A spectrogram recipe for ``StreamIndex.decode(..., features=spec)``; everything is validated here.

    ``n_fft``: a power of two from 128 to 4096 (the transform's plans; 400 is refused, not approximated).  ``hop >= 1``.
    ``win_length <= n_fft`` (default ``n_fft``), ``window``: "hann" (periodic), "hamming", "rect" or ``win_length`` weights.
    ``center``: frames centred on ``f * hop`` with zeros before row 0 (no reflection).  ``power``: 2 or 1.
    ``n_mels``: a triangular mel bank (``mel_filterbank``: ``fmin``, ``fmax``, ``mel="htk"|"slaney"``, ``norm=None|"slaney"``)
    built for the call's sample rate; or ``filterbank``: any dense ``[n_bins, n_fft/2 + 1]`` matrix, used as its rows' bands
    (first to last non-zero entry; zeros in between stay as weights).  ``log``: None, "ln", "log10" or "db" of ``max(v,
    floor)``, which needs ``floor > 0``.  ``dtype``: "f32" or "f64"."""

    def __init__(self, n_fft, hop, *, win_length=None, window="hann", center=False, power=2, n_mels=None, fmin=0.0, fmax=None,
                 mel="htk", norm=None, filterbank=None, log=None, floor=None, dtype="f32"):
        ints = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not ints(n_fft) or n_fft not in N_FFT:
            raise ValueError(f"n_fft is a power of two from 128 to 4096 (got {n_fft!r})")
        if not ints(hop) or hop < 1:
            raise ValueError(f"hop is at least 1 (got {hop!r})")
        win_length = n_fft if win_length is None else win_length
        if not ints(win_length) or not 1 <= win_length <= n_fft:
            raise ValueError(f"1 <= win_length <= n_fft (got {win_length!r})")
        if power not in (1, 2):
            raise ValueError(f"power is 1 or 2 (got {power!r})")
        if dtype not in ("f32", "f64"):
            raise ValueError(f"dtype is 'f32' or 'f64' (got {dtype!r})")
        if log not in (None,) + tuple(LOG_SCALE):
            raise ValueError(f"log is None, 'ln', 'log10' or 'db' (got {log!r})")
        if log is not None and not (floor is not None and np.isfinite(floor) and floor > 0):
            raise ValueError(f"a logarithm needs a finite floor > 0 (got {floor!r})")
        if floor is not None and not (np.isfinite(floor) and floor > 0):
            raise ValueError(f"floor is finite and > 0 (got {floor!r})")
        if n_mels is not None and filterbank is not None:
            raise ValueError("n_mels and filterbank exclude each other")
        self.n_fft, self.hop, self.win_length, self.center, self.power = int(n_fft), int(hop), int(win_length), bool(center), int(power)
        self.window = make_window(window, self.win_length, self.n_fft)
        self.log, self.floor, self.dtype = log, floor, np.dtype(np.float32 if dtype == "f32" else np.float64)
        self.n_mels, self.fmin, self.fmax, self.mel, self.norm = n_mels, float(fmin), fmax, mel, norm
        self._bands, self._cache = None, {}
        if n_mels is not None:
            if not ints(n_mels) or n_mels < 1:
                raise ValueError(f"n_mels is at least 1 (got {n_mels!r})")
            if mel not in ("htk", "slaney") or norm not in (None, "slaney"):
                raise ValueError(f"mel is 'htk' or 'slaney' and norm None or 'slaney' (got {mel!r}, {norm!r})")
            if fmin < 0 or (fmax is not None and not fmin < fmax):
                raise ValueError(f"the mel bank needs 0 <= fmin < fmax (got {fmin}, {fmax})")
        if filterbank is not None:
            try:
                bank = np.array(filterbank, np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"filterbank is not a float64 matrix: {e}") from None
            if bank.ndim != 2 or bank.shape[1] != n_fft // 2 + 1 or bank.shape[0] < 1:
                raise ValueError(f"filterbank must be [n_bins, {n_fft // 2 + 1}] (got {list(bank.shape)})")
            if not np.isfinite(bank).all():
                raise ValueError("filterbank is not finite")
            self._bands = bands_of(bank)

    @property
    def needs_rate(self) -> bool:
        return self.n_mels is not None

    def frames(self, rows: int) -> int:
        return frame_count(rows, self.n_fft, self.hop, self.center)

    def tables(self, srate=None) -> SpecTables:
        """the launch tables -- for a mel bank at ``srate`` (ValueError without one, or where fmax exceeds srate / 2)"""
        key = int(srate) if self.needs_rate and srate is not None else None
        if key not in self._cache:
            bands = self._bands
            if self.needs_rate:
                if not srate:
                    raise ValueError("a mel filterbank needs the sample rate: give srate=, or use streams of one rate")
                bands = bands_of(mel_filterbank(srate, self.n_fft, self.n_mels, self.fmin, self.fmax, self.mel, self.norm))
            self._cache[key] = SpecTables(self.n_fft, self.hop, self.center, self.power, self.window, bands,
                                          LOG_SCALE[self.log] if self.log else 0.0, self.floor, self.dtype, key=(id(self), key))
        return self._cache[key]


def clips_spectrum_host(x, spec, srate=None, rows=None) -> np.ndarray:
    """The definition in numpy for one window: ``x`` [valid, K] float64, ``spec`` a ``Spectral`` (``srate`` for its mel bank) or a
    ``SpecTables``; ``rows`` (default ``len(x)``): the length the frame count is taken from -- ``pad_to`` -- rows past ``len(x)``
    being zero.  -> ``[F, K, n_bins]`` of the spec's dtype.  ``np.fft.rfft`` in float64; the bank as a dense product; a clamped
    value is ``s * log(floor)`` as the tables hold it."""
    tb = spec.tables(srate) if isinstance(spec, Spectral) else spec
    x = np.asarray(x, np.float64)
    if x.ndim == 1:
        x = x[:, None]
    K = x.shape[1]
    rows = len(x) if rows is None else int(rows)
    F = frame_count(rows, tb.n_fft, tb.hop, tb.center)
    pad = tb.n_fft // 2 if tb.center else 0
    span = pad + max(rows, len(x)) + tb.n_fft + (F * tb.hop if F else 0)
    padded = np.zeros((span, K))
    padded[pad:pad + len(x)] = x
    at = np.arange(F)[:, None] * tb.hop + np.arange(tb.n_fft)[None, :]
    frames = padded[at] * tb.window[None, :, None]             # [F, n_fft, K]
    spec_c = np.fft.rfft(frames, axis=1)                       # [F, n_bins, K]
    with np.errstate(all="ignore"):
        P = spec_c.real * spec_c.real + spec_c.imag * spec_c.imag
        if tb.power == 1:
            P = np.sqrt(P)
        P = np.transpose(P, (0, 2, 1))                         # [F, K, n_bins]
        bank = tb.dense_bank()
        if bank is not None:
            P = P @ bank.T + 0.0                               # (an all-zero row gives +0.0, never -0.0)
        if tb.log_scale:
            P = np.where(P <= tb.floor, tb.floor_log, tb.log_scale * np.log(np.where(P <= tb.floor, tb.floor, P)))
    return np.ascontiguousarray(P).astype(tb.dtype)
