"""``StreamIndex`` and ``decode_windows``: sample windows of many streams decoded in one device pass.

A data loader takes a crop -- a second or two out of a file that is minutes long.  ``decode_batch`` and a slice on the host
give it, at the cost of the whole stream.  A FrAD stream is a sequence of self-contained frames, the header scan gives every
frame's place and geometry without the device, and an output sample depends on at most two frames: its own and, inside the
Hann cross-fade, the one before.  ``StreamIndex`` scans the streams once and keeps the per-stream plan of ``decode_batch``;
``index.decode`` selects the frames the windows need (merged per stream, so that overlapping windows share what is decoded for
them), sends the frames of ALL windows of a geometry group through each decode stage in one call, and one launch of
``frad_clips_window_add`` per group cross-fades, cuts, converts and writes every window -- ragged, or with ``pad_to`` scattered
into one dense zero-padded ``[B, T, C]`` batch.

Contract: ``res.pcm[k]`` of window ``(i, start, length)`` is bit for bit ``decode_batch([streams[i]], ...).pcm[0][start:start +
length]`` with the same keywords on the same bridge.  A stream that does not have the batched shape is decoded whole by a
per-stream ``Decoder``, as ``decode_batch`` does, sliced on the host and listed in ``res.fallback``.

``index.decode(..., srate=R)`` takes the windows from every stream resampled to R Hz: the source rows a window
reads are decoded as above, to float64 on the device, and one launch of ``frad_clips_resample`` per ratio -- ``scipy.signal.
resample_poly``'s arithmetic -- resamples, converts and writes them, so that streams of mixed rates give one dense batch.

``index.decode(..., channels=K)`` gives every window with K channels: the windows are decoded (and resampled) as
above, to float64 on the device, and one launch of ``frad_clips_remix`` per call applies each stream's matrix [K, C_in], converts
and writes them, so that mono and stereo streams give one dense [B, T, K] batch.

``index.decode(..., features=spec)`` returns spectrograms instead of samples (``spectral.Spectral``): the windows
are decoded, resampled and mixed as above, to float64 on the device, and one launch of ``frad_clips_spectrum`` per call frames,
windows and transforms them, applies the filterbank and the logarithm and writes ``[F, K, n_bins]`` per window or one dense
``[B, F, K, n_bins]`` batch."""
from __future__ import annotations

import functools
import math

import numpy as np

from .backend.pcmformat import ff_format_to_numpy_type, from_f64
from .batch import _frames, _plan, _scan_together, clips_overlap_host, decode_batch
from .frames import repair
from .spectral import Spectral, clips_spectrum_host


class WindowResult:
    """``pcm[k]`` [rows_k, channels] of window k; ``lengths[k]`` = rows_k; ``batch``: with ``pad_to=T`` the dense [B, T, C] block
    (``pcm[k]`` are then views into it), else None; ``fallback``: the sorted indices of the streams a per-stream ``Decoder``
    decoded.  With ``features=``: ``features[k]`` [frames_k, K, n_bins], ``frames[k]``, ``feature_batch`` [B, F, K, n_bins] with
    ``pad_to`` (else None), and ``pcm`` / ``batch`` are None unless ``keep_pcm``; without it the three are None."""

    def __init__(self, n: int):
        self.pcm = [None] * n
        self.lengths = [0] * n
        self.batch = None
        self.fallback = []
        self.features = self.frames = self.feature_batch = None


def select_frames(a: int, b: int, cut: int, L: int, m: int, has_tail: bool):
    """The frames rows [a, b), a < b, of a stream's timeline depend on -- m main frames ``cut`` apart that overlap by L rows, then
    the tail frame or the flush fragment.  -> (fa, fb, tail): main frames [fa, fb) and whether the tail frame is read.  A row
    reads its own frame and, in that frame's first L rows, the one before."""
    body = m * cut
    if a < body:
        fa = a // cut
        if fa > 0 and a % cut < L:
            fa -= 1
    elif has_tail and (a - body >= L or m == 0):
        fa = m
    else:
        fa = m - 1                                            # the tail's fade, or the flush fragment: rows of the last main frame
    if b <= body:
        return fa, (b - 1) // cut + 1, False
    return fa, m, has_tail


def merge_runs(ranges) -> list:
    """half-open ranges -> the sorted disjoint runs that cover them (ranges that touch are one run)"""
    runs = []
    for lo, hi in sorted(r for r in ranges if r[1] > r[0]):
        if runs and lo <= runs[-1][1]:
            runs[-1][1] = max(runs[-1][1], hi)
        else:
            runs.append([lo, hi])
    return runs


def clips_window_host(frames, clip_f0, clip_m, N, C, ratio, tails: list, tail_off, tail_rows, skip, valid, out_format=None):
    """What ``frad_clips_window_add`` computes without padding, with ``clips_overlap_host``'s arithmetic: rows ``skip[j] : skip[j] +
    valid[j]`` of the timeline of clip j (frames ``clip_f0[j] : clip_f0[j] + clip_m[j]``, the tail at ``tail_off[j]``), clip
    after clip.  For a bridge without ``clips_window_add``, and the kernel tests' model.  -> (ndarray [rows, C], out_off)"""
    flat = [np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in tails])] if tails else []
    pieces, out_off = [], [0]
    for j in range(len(clip_f0)):
        f0, m = int(clip_f0[j]), int(clip_m[j])
        whole, _ = clips_overlap_host(frames[f0:f0 + m] if m else None, [0, m], N, C, ratio, flat, [tail_off[j]], [tail_rows[j]])
        pieces.append(whole[int(skip[j]):int(skip[j]) + int(valid[j])])
        out_off.append(out_off[-1] + len(pieces[-1]))
    out = np.concatenate(pieces) if pieces else np.zeros((0, C))
    if out_format is not None:
        out = from_f64(out, out_format)
    return out, np.asarray(out_off, np.int64)


RESAMPLE_MAX = 2048                                            # max(up, down) of StreamIndex.decode(srate=): beyond it the taps are no table


def resample_ratio(srate_out: int, srate_in: int):
    """-> (up, down, half) of resampling ``srate_in`` to ``srate_out``: the reduced ratio, and the taps' half length 10 * max"""
    g = math.gcd(srate_out, srate_in)
    up, down = srate_out // g, srate_in // g
    return up, down, 10 * max(up, down)


@functools.lru_cache(maxsize=None)
def resample_taps(up: int, down: int) -> np.ndarray:
    """The 2 * half + 1 taps of ``scipy.signal.resample_poly(x, up, down)`` with default arguments, in float64 with numpy alone:
    firwin(2 * half + 1, 1 / M, window=("kaiser", 5.0)) * up, M = max(up, down), half = 10 * M.  Read-only (it is cached)."""
    M = max(up, down)
    half = 10 * M
    h = np.sinc((np.arange(2 * half + 1) - half) / M) / M * np.kaiser(2 * half + 1, 5.0)
    h = h / h.sum() * up
    h.setflags(write=False)
    return h


def resample_rows(n_in: int, up: int, down: int) -> int:
    """rows of ``n_in`` rows resampled by up / down: ceil(n_in * up / down)"""
    return -(-n_in * up // down)


def resample_needs(a: int, b: int, up: int, down: int, n_in: int):
    """-> the source rows [lo, hi) that output rows [a, b) of the resampled stream read, clipped to the stream's ``n_in`` rows"""
    if a >= b:
        return 0, 0
    half = 10 * max(up, down)
    lo = max(0, -(-(a * down - half) // up))
    hi = min(n_in, ((b - 1) * down + half) // up + 1)
    return (lo, hi) if hi > lo else (0, 0)


def clips_resample_host(src, src_off, src_row0, src_rows, C, up, down, out_row0, valid, out_format=None):
    """What ``frad_clips_resample`` computes without padding, in numpy: rows ``out_row0[j] : out_row0[j] + valid[j]`` of the
    stream resampled by ``up / down``, from the ``src_rows[j]`` source rows at element ``src_off[j]`` of the flat float64 ``src``
    that are rows ``src_row0[j] ..`` of the stream (rows outside count as zero), clip after clip.  The definition is the entry
    point's (include/frad_hip.h): the terms in ascending source order from 0.0, with a multiply and an add in place of the fma.
    For a bridge without ``clips_resample``, and the kernel tests' model.  -> (ndarray [rows, C], out_off)"""
    src = np.asarray(src, np.float64).reshape(-1)
    h = resample_taps(up, down)
    half = 10 * max(up, down)
    terms = 2 * half // up + 1
    pieces, out_off = [], [0]
    for j in range(len(src_off)):
        rows, s0 = int(src_rows[j]), int(src_row0[j])
        x = src[int(src_off[j]):int(src_off[j]) + rows * C].reshape(rows, C)
        n = int(out_row0[j]) + np.arange(int(valid[j]), dtype=np.int64)
        lo = np.maximum(np.maximum(-(-(n * down - half) // up), 0), s0)
        hi = np.minimum((n * down + half) // up, s0 + rows - 1)
        acc = np.zeros((len(n), C))
        for t in range(terms):
            i = lo + t
            live = i <= hi
            if not live.any():
                break
            at = np.where(live, i - s0, 0)
            k = np.where(live, n * down - i * up + half, 0)
            acc = np.where(live[:, None], acc + x[at] * h[k][:, None], acc) if rows else acc
        pieces.append(acc)
        out_off.append(out_off[-1] + len(acc))
    out = np.concatenate(pieces) if pieces else np.zeros((0, C))
    if out_format is not None:
        out = from_f64(out, out_format)
    return out, np.asarray(out_off, np.int64)


def remix_matrix(c_in: int, channels: int):
    """The float64 matrix [channels, c_in] of ``StreamIndex.decode(channels=)`` for a stream of ``c_in`` channels: the identity
    for ``c_in == channels``, the mean (every weight ``1.0 / c_in``) for one output channel, the mono channel copied to every
    output channel for ``c_in == 1`` -- and None for anything else: the project does not invent down-mix coefficients."""
    if c_in == channels:
        return np.eye(channels)
    if channels == 1:
        return np.full((1, c_in), 1.0 / c_in)
    if c_in == 1:
        return np.ones((channels, 1))
    return None


def clips_remix_host(x, matrix, out_format=None):
    """What ``frad_clips_remix`` computes for one clip, in numpy: rows ``x`` [rows, C_in] mixed by ``matrix`` [K, C_in] -> [rows, K].
    The definition is the entry point's (include/frad_hip.h): for output channel k the terms are the c, ascending, with
    ``matrix[k][c] != 0.0``; the first sets the sum, every later one is a rounded multiply and a rounded add; a row of the matrix
    without a non-zero entry gives +0.0.  For a bridge without ``clips_remix``, and the kernel tests' model."""
    x = np.asarray(x, np.float64)
    m = np.asarray(matrix, np.float64)
    x = x.reshape(-1, m.shape[1])
    out = np.zeros((len(x), m.shape[0]))
    with np.errstate(all="ignore"):
        for k in range(m.shape[0]):
            first = True
            for c in range(m.shape[1]):
                if m[k, c] == 0.0:
                    continue
                p = x[:, c] * m[k, c]
                out[:, k] = p if first else out[:, k] + p
                first = False
    return out if out_format is None else from_f64(out, out_format)


class StreamIndex:
    """The frame index of a set of complete streams: one header scan (``frad_asfh_scan`` over all of them, no device work) and the
    per-stream plan of ``decode_batch``, kept for any number of ``decode`` calls.  ``fix_error`` belongs to the index: how a
    protected frame is classified depends on it.

    ``samples[i]``: the rows ``decode_batch`` returns for stream i, from the headers alone -- None for a stream that does not
    have the batched shape (``fallback`` lists those; what is known of them is known only after decoding).  ``srate[i]``,
    ``channels[i]`` (of the last header), ``frames[i]``: as ``BatchResult`` gives them, None for a fallback stream."""

    def __init__(self, streams, *, fix_error: bool = False, bridge=None):
        if bridge is None:
            from .bridge import HipBridge
            bridge = HipBridge()
        self.bridge, self.fix_error = bridge, fix_error
        self.streams = [s if isinstance(s, bytes) else bytes(s) for s in streams]
        n = len(self.streams)
        scan_lib = getattr(bridge, "scan_lib", None)
        if scan_lib is None or not n:
            self.plans = [None] * n                            # no native scanner behind this bridge: every stream on its own
        else:
            joined, rows_of = _scan_together(scan_lib.asfh_scan, self.streams)
            self.plans = [_plan(rows, joined, fix_error) if rows is not None else None for rows in rows_of]
        self.samples, self.srate, self.channels, self.frames = ([None] * n for _ in range(4))
        self.fallback = [i for i, p in enumerate(self.plans) if p is None]
        for i, p in enumerate(self.plans):
            if p is not None:
                self.samples[i] = sum(self._geometry(p)[4:]) if p.key is not None else 0
                self.srate[i], self.channels[i], self.frames[i] = p.srate, p.channels, p.frames

    @staticmethod
    def _geometry(p):
        """-> (cut, L, m, tail rows R, body = m * cut, rows behind the body) of a planned stream with frames"""
        N, ratio = p.key[1], p.key[6]
        cut = N * (ratio - 1) // ratio if ratio else N
        m = len(p.main)
        R = p.tail_key[1] if p.tail_key is not None else 0
        return cut, N - cut, m, R, m * cut, R if R else (N - cut if m else 0)

    def samples_at(self, srate: int) -> list:
        """``samples`` at ``srate``: the rows of every stream resampled to it, ceil(samples * up / down), from the headers alone
        -- None for a fallback stream"""
        if srate < 1:
            raise ValueError(f"a sample rate is at least 1 (got {srate})")
        out = []
        for i, p in enumerate(self.plans):
            if p is None or (self.samples[i] and not p.srate):
                out.append(None)
            elif not self.samples[i] or p.srate == srate:
                out.append(self.samples[i])
            else:
                up, down, _ = resample_ratio(srate, p.srate)
                out.append(resample_rows(self.samples[i], up, down))
        return out

    def decode(self, windows, *, pad_to: int | None = None, out_format: str | None = None, device_inflate: bool = False,
               as_tensor: bool = False, max_batch_bytes: int = 1 << 30, srate: int | None = None, channels: int | None = None,
               mix: dict | None = None, features: Spectral | None = None, keep_pcm: bool = False) -> WindowResult:
        """Decode ``windows``, a sequence of ``(stream, start, length)``: rows ``start : start + length`` of stream ``stream`` of
        the index (``length`` None: to the end; a window is clipped to the stream's end; a stream may be named any number of
        times).  ``out_format``, ``device_inflate``, ``as_tensor`` and ``max_batch_bytes`` mean what they mean for
        ``decode_batch`` (a group is cut into chunks of whole windows).  ``pad_to=T``: ``res.batch`` is the dense block
        [len(windows), T, C] -- an ndarray of ``out_format``'s dtype (float64 without one), or with ``as_tensor`` a device tensor
        (float64, or the uint8 bytes [B, T, C * itemsize] of ``out_format``) -- rows past ``res.lengths[k]`` hold the format's
        silence, and ``res.pcm[k]`` are views into it; ValueError when the streams used differ in channel count or a window is
        longer than T.

        ``srate=R``: the windows are taken from every stream resampled to R Hz -- ``start``, ``length`` and ``pad_to`` count
        rows at R, ``samples_at(R)`` gives the streams' lengths.  The arithmetic is ``scipy.signal.resample_poly``'s (polyphase,
        zero extension, Kaiser beta = 5; include/frad_hip.h, frad_clips_resample): the source rows a window reads are decoded to
        float64 by the path above and one ``frad_clips_resample`` per ratio resamples, converts and writes them, so a window is
        bit for bit the slice of the whole resampled stream.  A stream whose rate is R is not touched: its windows are byte for
        byte those of the call without ``srate``.  ValueError for R < 1 and for a ratio whose reduced max(up, down) is beyond
        2048.

        ``channels=K``: every window has K channels, whatever its stream has.  A stream of ``C_in`` channels is
        mixed by a float64 matrix [K, C_in]: the identity for ``C_in == K``, the mean for K = 1, the mono channel copied K times
        for ``C_in == 1``; anything else needs ``mix={C_in: matrix}``, which also overrides the rule for that ``C_in``
        (``mix`` alone: K is the matrices' own, and every stream used needs an entry).  The order is decode, resample, mix,
        ``out_format``: the windows are decoded (and resampled) to float64 as above, and one ``frad_clips_remix`` mixes,
        converts, pads and writes all of them -- ``res.pcm[k]`` is bit for bit ``from_f64(clips_remix_host(X_k, M), out_format)``
        of the float64 window ``X_k`` the call without ``channels`` and ``out_format`` gives -- so ``pad_to`` takes streams of
        mixed channel counts: ``res.batch`` is [B, T, K].  ValueError, before anything is decoded, for K < 1, a matrix that is not
        finite, not [K, C_in] or of another K, and a stream without a matrix (a fallback stream's channel count is known only
        once it is decoded: for it the last is raised then, before anything is mixed).

        ``features=spec`` (a ``spectral.Spectral``): the result is the spectrogram of every window.  The order is
        decode, resample, mix, features: the spectral stage reads the float64 windows ``X_k`` [rows_k, K] that the same call
        without ``features`` gives, rows outside a window counting as zero, and one ``frad_clips_spectrum`` writes all of them:
        ``res.features[k]`` is ``[frames_k, K, n_bins]`` of the spec's dtype -- ``spectral.clips_spectrum_host(X_k, spec)`` within
        the transform's float64 rounding -- and ``res.frames[k]`` the frame count of the window's own length
        (``spec.frames(rows_k)``).  With ``pad_to=T`` every window has ``F = spec.frames(T)`` frames, ``res.feature_batch`` is the
        dense ``[B, F, K, n_bins]`` block (``.permute(0, 2, 3, 1)`` is torch's ``[B, K, n_bins, F]``, a view) and
        ``res.features[k]`` its first ``frames_k`` frames, bit for bit those of the ragged call.  The streams used need one
        channel count (``channels=`` gives it).  A mel bank is built for ``srate``, else for the one rate of the streams used.
        ``res.pcm`` and ``res.batch`` are None unless ``keep_pcm``: then they are those of the call without ``features``.
        ValueError, before anything is decoded, for ``out_format`` together with ``features``, ``pad_to < n_fft`` without
        ``center``, streams of several rates under a mel bank without ``srate``, a mel bank whose ``fmax`` is beyond half the
        rate, and streams of several channel counts (for a fallback stream what depends on the stream is raised once it is
        decoded).  ``keep_pcm`` without ``features`` is a ValueError too."""
        if features is not None:
            return self._decode_features(features, keep_pcm, windows, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes, srate,
                                         channels, mix)
        if keep_pcm:
            raise ValueError("keep_pcm goes with features")
        if channels is not None or mix is not None:
            return self._decode_mixed(windows, channels, mix, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes, srate)
        if srate is not None:
            return self._decode_at(srate, windows, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes)
        br = self.bridge
        dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
        if as_tensor and getattr(br, "torch", None) is None:
            raise ValueError("as_tensor needs a bridge that keeps tensors on the device")
        wins = []
        for i, start, length in windows:
            if not 0 <= i < len(self.streams):
                raise IndexError(f"stream {i} is not in the index")
            if start < 0 or (length is not None and length < 0):
                raise ValueError(f"a window needs start >= 0 and length >= 0 (got {start}, {length})")
            wins.append((i, start, length))
        res = WindowResult(len(wins))
        kw = dict(fix_error=self.fix_error, out_format=out_format, device_inflate=device_inflate, bridge=br)
        whole = {i: decode_batch([self.streams[i]], **kw).pcm[0] for i in sorted({w[0] for w in wins if self.plans[w[0]] is None})}
        res.fallback = sorted(whole)
        # ---- every window as rows [a, b) of its stream, clipped; the ones a launch writes, by geometry key
        spans, groups, channels = [], {}, set()
        for k, (i, start, length) in enumerate(wins):
            p = self.plans[i]
            total = len(whole[i]) if p is None else self.samples[i]
            a = min(start, total)
            b = total if length is None else max(a, min(start + length, total))
            spans.append((a, b))
            res.lengths[k] = b - a
            channels.add(whole[i].shape[1] if p is None else p.channels)
            if p is not None and p.key is not None and (b > a or pad_to is not None):
                groups.setdefault(p.key, []).append(k)
        on_dev = getattr(br, "clips_window_add", None)
        dense = None
        if pad_to is not None:
            if len(channels) > 1:
                raise ValueError(f"a dense batch needs one channel count (the streams used have {sorted(channels)})")
            if any(n > pad_to for n in res.lengths):
                raise ValueError(f"a window is longer than pad_to = {pad_to}")
            C = channels.pop() if channels else 0
            if on_dev is not None:                             # the launches scatter into it; what no launch writes is filled below
                t = br.torch
                dense = t.empty((len(wins), pad_to, C), dtype=t.float64, device=br.device) if out_format is None else \
                    t.empty((len(wins), pad_to, C * dt.itemsize), dtype=t.uint8, device=br.device)
            else:
                dense = np.empty((len(wins), pad_to, C), dt)

        def finish(k, pcm):
            if as_tensor and isinstance(pcm, np.ndarray):
                t = br.torch
                raw = np.ascontiguousarray(pcm)
                pcm = t.from_numpy(raw if out_format is None else raw.view(np.uint8).reshape(-1)).to(br.device)
            res.pcm[k] = pcm

        launched = set()

        def run(key, chunk, needs_of):
            self._decode_chunk(key, chunk, wins, spans, needs_of, finish, dense, pad_to, out_format, device_inflate, as_tensor)
            launched.update(chunk)

        for key, members in groups.items():
            chunk, needs_of, bytes_of, size = [], {}, {}, 0    # needs_of[i]: the (fa, fb, tail) of stream i's windows in the chunk
            for k in members:
                i = wins[k][0]
                need = self._needs(i, *spans[k])
                grown = needs_of.get(i, []) + [need]
                if chunk and size - bytes_of.get(i, 0) + self._bytes(i, grown) > max_batch_bytes:
                    run(key, chunk, needs_of)
                    chunk, needs_of, bytes_of, size, grown = [], {}, {}, 0, [need]
                chunk.append(k)
                size -= bytes_of.get(i, 0)
                needs_of[i], bytes_of[i] = grown, self._bytes(i, grown)
                size += bytes_of[i]
            run(key, chunk, needs_of)
        # ---- the windows no launch wrote: a fallback stream's slice, and the empty ones
        silence = from_f64(np.zeros(1), dt)
        for k, (i, start, length) in enumerate(wins):
            if k in launched:
                continue
            a, b = spans[k]
            piece = whole[i][a:b] if self.plans[i] is None else np.zeros((0, self.plans[i].channels), dt)
            if dense is None:
                finish(k, piece)
                continue
            host = isinstance(dense, np.ndarray)
            row = dense[k] if host else np.empty((pad_to, C), dt)
            row[:b - a] = piece
            row[b - a:] = silence
            if not host:
                dense[k] = br.torch.from_numpy(row if out_format is None else row.view(np.uint8)).to(br.device)
        if dense is not None:
            if not as_tensor and not isinstance(dense, np.ndarray):
                dense = dense.cpu().numpy().view(dt)           # one download of the whole batch
            res.batch = dense
            for k in range(len(wins)):
                view = dense[k, :res.lengths[k]]
                res.pcm[k] = view.reshape(-1) if as_tensor and out_format is not None else view
        return res

    # -------------------------------------------------------------------------------------------- windows at one sample rate
    def _decode_at(self, R, windows, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes) -> WindowResult:
        """``decode`` with ``srate=R``: the windows of streams at R through ``decode`` itself, the others as source windows
        through ``decode`` (float64, on the device where the bridge keeps tensors) and then one ``clips_resample`` per ratio and
        channel count."""
        br = self.bridge
        if R < 1:
            raise ValueError(f"a sample rate is at least 1 (got {R})")
        dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
        on_dev = getattr(br, "clips_resample", None)
        if as_tensor and getattr(br, "torch", None) is None:
            raise ValueError("as_tensor needs a bridge that keeps tensors on the device")
        wins = []
        for i, start, length in windows:
            if not 0 <= i < len(self.streams):
                raise IndexError(f"stream {i} is not in the index")
            if start < 0 or (length is not None and length < 0):
                raise ValueError(f"a window needs start >= 0 and length >= 0 (got {start}, {length})")
            wins.append((i, start, length))
        res = WindowResult(len(wins))
        kw = dict(device_inflate=device_inflate, max_batch_bytes=max_batch_bytes)
        # ---- a fallback stream is decoded whole, to float64: its rate and length are known only then
        whole, rate, rows_in, chans = {}, {}, {}, {}
        for i in sorted({w[0] for w in wins}):
            p = self.plans[i]
            if p is None:
                got = decode_batch([self.streams[i]], fix_error=self.fix_error, device_inflate=device_inflate, bridge=br)
                whole[i], rate[i] = np.ascontiguousarray(got.pcm[0], np.float64), got.srate[0]
                rows_in[i], chans[i] = whole[i].shape
            else:
                rate[i], rows_in[i], chans[i] = p.srate, self.samples[i], p.channels
        res.fallback = sorted(whole)
        ratio = {}
        for i in rate:
            if rows_in[i] and rate[i] != R:
                if not rate[i]:
                    raise ValueError(f"stream {i} does not say its sample rate")
                ratio[i] = resample_ratio(R, rate[i])[:2]
                if max(ratio[i]) > RESAMPLE_MAX:
                    raise ValueError(f"resampling {rate[i]} Hz to {R} Hz needs {ratio[i][0]}/{ratio[i][1]}: beyond {RESAMPLE_MAX}")
        # ---- every window as rows [a, b) of its resampled stream, clipped, and the source rows [lo, hi) those read
        spans, needs = [], []
        for k, (i, start, length) in enumerate(wins):
            total = resample_rows(rows_in[i], *ratio[i]) if i in ratio else rows_in[i]
            a = min(start, total)
            b = total if length is None else max(a, min(start + length, total))
            spans.append((a, b))
            res.lengths[k] = b - a
            needs.append(resample_needs(a, b, *ratio[i], rows_in[i]) if i in ratio else (a, b))
        if pad_to is not None:
            if len({chans[i] for i, _, _ in wins}) > 1:
                raise ValueError(f"a dense batch needs one channel count (the streams used have {sorted({chans[i] for i, _, _ in wins})})")
            if any(n > pad_to for n in res.lengths):
                raise ValueError(f"a window is longer than pad_to = {pad_to}")
        same = [k for k, w in enumerate(wins) if w[0] not in ratio]
        other = [k for k, w in enumerate(wins) if w[0] in ratio]
        dense = None
        if pad_to is not None:
            C = chans[wins[0][0]] if wins else 0
            if on_dev is not None:
                t = br.torch
                dense = t.empty((len(wins), pad_to, C), dtype=t.float64, device=br.device) if out_format is None else \
                    t.empty((len(wins), pad_to, C * dt.itemsize), dtype=t.uint8, device=br.device)
            else:
                dense = np.empty((len(wins), pad_to, C), dt)
        # ---- the streams at R: the path without srate, with the caller's own windows
        if same:
            keep = as_tensor if dense is None else not isinstance(dense, np.ndarray)     # (a device batch is filled on the device)
            got = self.decode([wins[k] for k in same], pad_to=pad_to, out_format=out_format, as_tensor=keep, **kw)
            if dense is None:
                for n, k in enumerate(same):
                    res.pcm[k] = got.pcm[n]
            elif isinstance(dense, np.ndarray):
                dense[same] = got.batch
            else:
                dense[br.torch.as_tensor(same, device=br.device)] = got.batch
        # ---- the others: their source rows as float64 (planned streams: one more decode; fallback streams: the whole stream
        # once, shared by its windows), then one clips_resample per (up, down, channels)
        planned = [k for k in other if self.plans[wins[k][0]] is not None and needs[k][1] > needs[k][0]]
        pieces = {}
        if planned:
            got = self.decode([(wins[k][0], needs[k][0], needs[k][1] - needs[k][0]) for k in planned], as_tensor=on_dev is not None, **kw)
            pieces = {k: got.pcm[n] for n, k in enumerate(planned)}
        groups = {}
        for k in other:
            i = wins[k][0]
            groups.setdefault(ratio[i] + (chans[i],), []).append(k)
        for (up, down, C), members in groups.items():
            parts, at, placed = [], 0, {}
            n = len(members)
            src_off, src_row0, src_rows = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
            out_row0, valid = np.zeros(n, np.int64), np.zeros(n, np.int32)
            for j, k in enumerate(members):
                i, (a, b), (lo, hi) = wins[k][0], spans[k], needs[k]
                out_row0[j], valid[j] = a, b - a
                if hi <= lo:
                    continue
                if i in whole:                                # the whole stream is one span, placed once
                    if i not in placed:
                        placed[i] = at
                        parts.append(whole[i].reshape(-1))
                        at += whole[i].size
                    src_off[j], src_row0[j], src_rows[j] = placed[i], 0, rows_in[i]
                else:
                    src_off[j], src_row0[j], src_rows[j] = at, lo, hi - lo
                    parts.append(pieces[k].reshape(-1))
                    at += (hi - lo) * C
            if on_dev is None:
                src = np.concatenate([np.asarray(x, np.float64) for x in parts]) if parts else np.zeros(0)
                out, out_off = clips_resample_host(src, src_off, src_row0, src_rows, C, up, down, out_row0, valid, out_format)
                for j, k in enumerate(members):
                    piece = out[int(out_off[j]):int(out_off[j + 1])]
                    if dense is None:
                        res.pcm[k] = piece
                    else:
                        dense[k, :len(piece)] = piece
                        dense[k, len(piece):] = from_f64(np.zeros(1), dense.dtype)
                continue
            t = br.torch
            parts = [x if isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x, np.float64)).to(br.device) for x in parts]
            src = None if not parts else parts[0] if len(parts) == 1 else t.cat(parts)
            if dense is not None:
                on_dev(src, src_off, src_row0, src_rows, C, up, down, out_row0, valid, out_format, span=np.full(n, pad_to, np.int64),
                       dst_row=np.asarray(members, np.int64) * pad_to, out=dense)
                continue
            out, out_off = on_dev(src, src_off, src_row0, src_rows, C, up, down, out_row0, valid, out_format, as_tensor=as_tensor)
            step = C * dt.itemsize if as_tensor and out_format is not None else 1
            for j, k in enumerate(members):
                res.pcm[k] = out[int(out_off[j]) * step:int(out_off[j + 1]) * step]
        if dense is not None:
            if not as_tensor and not isinstance(dense, np.ndarray):
                dense = dense.cpu().numpy().view(dt)           # one download of the whole batch
            res.batch = dense
            for k in range(len(wins)):
                view = dense[k, :res.lengths[k]]
                res.pcm[k] = view.reshape(-1) if as_tensor and out_format is not None else view
        return res

    # ------------------------------------------------------------------------------------------- windows of K channels each
    def _decode_mixed(self, windows, channels, mix, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes, srate) -> WindowResult:
        """``decode`` with ``channels`` or ``mix``: the windows as float64 through ``decode`` itself (on the device where the
        bridge keeps tensors), then one ``clips_remix`` that mixes, converts, pads and writes all of them."""
        br = self.bridge
        # ---- the arguments, before anything is decoded
        if channels is not None and (isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or channels < 1):
            raise ValueError(f"channels is a count of at least 1 (got {channels!r})")
        given = {}
        for c_in, m in (mix or {}).items():
            if isinstance(c_in, bool) or not isinstance(c_in, (int, np.integer)) or c_in < 1:
                raise ValueError(f"mix is keyed by channel counts (got {c_in!r})")
            try:
                m = np.array(m, np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"mix[{c_in}] is not a float64 matrix: {e}") from None
            if m.ndim != 2 or m.shape[1] != c_in or m.shape[0] < 1:
                raise ValueError(f"mix[{c_in}] must be a matrix [channels, {c_in}] (got {list(m.shape)})")
            if not np.isfinite(m).all():
                raise ValueError(f"mix[{c_in}] is not finite")
            given[int(c_in)] = m
        K = int(channels) if channels is not None else None
        for c_in, m in given.items():
            if K is None:
                K = m.shape[0]
            if m.shape[0] != K:
                raise ValueError(f"mix[{c_in}] gives {m.shape[0]} channels, not {K}")
        if K is None:
            raise ValueError("mix is empty and channels is not given")
        if as_tensor and getattr(br, "torch", None) is None:
            raise ValueError("as_tensor needs a bridge that keeps tensors on the device")
        if srate is not None and srate < 1:
            raise ValueError(f"a sample rate is at least 1 (got {srate})")
        wins = []
        for i, start, length in windows:
            if not 0 <= i < len(self.streams):
                raise IndexError(f"stream {i} is not in the index")
            if start < 0 or (length is not None and length < 0):
                raise ValueError(f"a window needs start >= 0 and length >= 0 (got {start}, {length})")
            wins.append((i, start, length))
        mats = {}

        def matrix(i, c_in):
            if c_in not in mats:
                m = given.get(c_in)
                if m is None and channels is not None:
                    m = remix_matrix(c_in, K)
                if m is None:
                    raise ValueError(f"stream {i} has {c_in} channels: mix has no matrix [{K}, {c_in}] for it")
                mats[c_in] = m
            return mats[c_in]

        for i in sorted({w[0] for w in wins}):
            if self.plans[i] is not None:
                matrix(i, self.plans[i].channels)
        if pad_to is not None:                                 # (a fallback stream's length is known once it is decoded: below)
            totals = self.samples if srate is None else self.samples_at(srate)
            if any(totals[i] is not None and min(totals[i] - min(start, totals[i]), totals[i] if length is None else length) > pad_to
                   for i, start, length in wins):
                raise ValueError(f"a window is longer than pad_to = {pad_to}")
        # ---- the windows as float64, ragged
        dt = np.dtype(np.float64) if out_format is None else ff_format_to_numpy_type(out_format)
        on_dev = getattr(br, "clips_remix", None)
        got = self.decode(wins, device_inflate=device_inflate, max_batch_bytes=max_batch_bytes, srate=srate,
                          as_tensor=getattr(br, "torch", None) is not None)
        n = len(wins)
        res = WindowResult(n)
        res.lengths, res.fallback = got.lengths, got.fallback
        for k in range(n):
            matrix(wins[k][0], int(got.pcm[k].shape[1]))
        if pad_to is not None and any(rows > pad_to for rows in res.lengths):
            raise ValueError(f"a window is longer than pad_to = {pad_to}")
        # ---- the mix: the only conversion to out_format, and the only stage that writes the result
        if on_dev is None:
            pieces = [clips_remix_host(np.asarray(x), mats[int(x.shape[1])], out_format) for x in got.pcm]
            if pad_to is None:
                res.pcm = pieces
                return res
            res.batch = np.empty((n, pad_to, K), dt)
            silence = from_f64(np.zeros(1), dt)
            for k, piece in enumerate(pieces):
                res.batch[k, :len(piece)] = piece
                res.batch[k, len(piece):] = silence
                res.pcm[k] = res.batch[k, :len(piece)]
            return res
        t = br.torch
        valid = np.asarray(res.lengths, np.int32)
        if pad_to is None:
            if n:
                out, out_off = on_dev(got.pcm, mats, K, valid, out_format, as_tensor=as_tensor)
                step = K * dt.itemsize if as_tensor and out_format is not None else 1
                for k in range(n):
                    res.pcm[k] = out[int(out_off[k]) * step:int(out_off[k + 1]) * step]
            return res
        dense = t.empty((n, pad_to, K), dtype=t.float64, device=br.device) if out_format is None else \
            t.empty((n, pad_to, K * dt.itemsize), dtype=t.uint8, device=br.device)
        if n and pad_to:
            on_dev(got.pcm, mats, K, valid, out_format, span=np.full(n, pad_to, np.int64), dst_row=np.arange(n, dtype=np.int64) * pad_to,
                   out=dense)
        if not as_tensor:
            dense = dense.cpu().numpy().view(dt)               # one download of the whole batch
        res.batch = dense
        for k in range(n):
            view = dense[k, :res.lengths[k]]
            res.pcm[k] = view.reshape(-1) if as_tensor and out_format is not None else view
        return res

    # ---------------------------------------------------------------------------------------------- spectrograms of the windows
    def _decode_features(self, spec, keep_pcm, windows, pad_to, out_format, device_inflate, as_tensor, max_batch_bytes, srate, channels,
                         mix) -> WindowResult:
        """``decode`` with ``features``: the windows as float64 through ``decode`` itself (on the device where the bridge keeps
        tensors), then one ``clips_spectrum`` over all of them."""
        br = self.bridge
        # ---- the arguments, before anything is decoded
        if not isinstance(spec, Spectral):
            raise ValueError(f"features is a spectral.Spectral (got {type(spec).__name__})")
        if out_format is not None:
            raise ValueError("features reads the float64 windows: out_format does not go with it")
        if pad_to is not None and not spec.center and pad_to < spec.n_fft:
            raise ValueError(f"pad_to = {pad_to} is shorter than one frame of n_fft = {spec.n_fft}")
        on_torch = getattr(br, "torch", None) is not None
        if as_tensor and not on_torch:
            raise ValueError("as_tensor needs a bridge that keeps tensors on the device")
        if srate is not None and srate < 1:
            raise ValueError(f"a sample rate is at least 1 (got {srate})")
        wins = [tuple(w) for w in windows]
        used = sorted({w[0] for w in wins if isinstance(w[0], (int, np.integer)) and 0 <= w[0] < len(self.streams)})
        planned = [i for i in used if self.plans[i] is not None]
        rate = srate
        if spec.needs_rate and srate is None:
            rates = {self.plans[i].srate or None for i in planned} | ({None} if len(planned) < len(used) else set())
            if len(rates) > 1 or None in rates:                # (a fallback stream's rate is not known from its headers)
                raise ValueError(f"a mel filterbank needs one known sample rate (the streams used have {sorted(rates, key=str)}): give srate=")
            rate = rates.pop() if rates else None
        tb = spec.tables(rate) if not spec.needs_rate or rate else None          # (None: a mel bank and no stream, nothing to compute)
        n_bins = tb.n_bins if tb is not None else spec.n_mels
        if channels is None and mix is None and len({self.plans[i].channels for i in planned}) > 1:
            raise ValueError(f"features need one channel count (the streams used have {sorted({self.plans[i].channels for i in planned})}): "
                             "give channels=")
        # ---- the windows as float64: ragged, or the dense batch whose rows past a window's length are zero
        got = self.decode(wins, pad_to=pad_to, device_inflate=device_inflate, max_batch_bytes=max_batch_bytes, srate=srate,
                          channels=channels, mix=mix, as_tensor=on_torch)
        n = len(wins)
        res = WindowResult(n)
        res.lengths, res.fallback = got.lengths, got.fallback
        chans = {int(x.shape[1]) for x in got.pcm}
        if len(chans) > 1:
            raise ValueError(f"features need one channel count (the streams used have {sorted(chans)}): give channels=")
        K = chans.pop() if chans else (int(got.batch.shape[2]) if got.batch is not None else 0)
        res.frames = [spec.frames(rows) for rows in res.lengths]
        F = spec.frames(pad_to) if pad_to is not None else None
        counts = res.frames if F is None else [F] * n
        off = np.zeros(n + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        if keep_pcm:
            down = (lambda x: x) if as_tensor or not on_torch else (lambda x: x.cpu().numpy())
            if got.batch is not None:
                res.batch = down(got.batch)
                res.pcm = [res.batch[k, :res.lengths[k]] for k in range(n)]
            else:
                res.pcm = [down(x) for x in got.pcm]
        else:
            res.pcm = None
        # ---- the spectral stage: the only one that writes the result
        on_dev = getattr(br, "clips_spectrum", None)
        if on_dev is None:
            pieces = [clips_spectrum_host(np.asarray(x), tb, rows=pad_to) for x in got.pcm]
            flat = np.concatenate(pieces) if pieces else np.zeros((0, K, n_bins), spec.dtype)
        elif n and off[-1] and K:
            flat = on_dev(got.pcm, np.asarray(res.lengths, np.int32), tb, K, off)
            if not as_tensor:
                flat = flat.cpu().numpy()                      # one download of the whole result
        elif as_tensor:
            flat = br.torch.empty((0, K, n_bins), dtype=br.torch.float32 if spec.dtype == np.float32 else br.torch.float64, device=br.device)
        else:
            flat = np.zeros((0, K, n_bins), spec.dtype)
        if F is None:
            res.features = [flat[int(off[k]):int(off[k + 1])] for k in range(n)]
        else:
            res.feature_batch = flat.reshape(n, F, K, n_bins)
            res.features = [res.feature_batch[k, :min(res.frames[k], F)] for k in range(n)]
        return res

    # ------------------------------------------------------------------------------------------------ what a window needs
    def _needs(self, i: int, a: int, b: int):
        """-> (fa, fb, tail) of rows [a, b) of planned stream i; an empty window needs nothing"""
        if a >= b:
            return 0, 0, False
        cut, L, m, R, _, _ = self._geometry(self.plans[i])
        return select_frames(a, b, cut, L, m, R > 0)

    def _bytes(self, i: int, needs: list) -> int:
        """float64 bytes of the frames decoded for stream i when its windows need ``needs``: the merged runs, and the tail if read"""
        p = self.plans[i]
        N, C = p.key[1], p.key[2]
        return (sum(hi - lo for lo, hi in merge_runs((fa, fb) for fa, fb, _ in needs)) * N
                + (p.tail_key[1] if any(t for _, _, t in needs) else 0)) * C * 8

    def _decode_chunk(self, key, chunk, wins, spans, needs_of, finish, dense, pad_to, out_format, device_inflate, as_tensor):
        """The windows ``chunk`` of one geometry group: every stage once over the merged frame runs of their streams, the tails
        grouped by their size, then one ``clips_window_add``."""
        br = self.bridge
        N, C, ratio = key[1], key[2], key[6]
        cut = N * (ratio - 1) // ratio if ratio else N
        main, place, tails_by = [], {}, {}
        for i, needs in needs_of.items():                      # place[i]: [(lo, hi, the run's first frame in `main`)]
            p = self.plans[i]
            place[i] = []
            for lo, hi in merge_runs((fa, fb) for fa, fb, _ in needs):
                place[i].append((lo, hi, len(main)))
                main.extend(p.main[lo:hi])
            if any(t for _, _, t in needs):
                tails_by.setdefault(p.tail_key, []).append(i)
        order = [i for members in tails_by.values() for i in members]
        fixed = repair(br, main + [self.plans[i].tail for i in order])
        main, tail_payloads = fixed[:len(main)], fixed[len(main):]
        frames = _frames(br, key, main, device_inflate) if main else None
        tails, tail_at, off, at = [], {}, 0, 0
        for tkey, members in tails_by.items():                 # the last frames, grouped again by their size
            tails.append(_frames(br, tkey, tail_payloads[at:at + len(members)], device_inflate))
            at += len(members)
            for n, i in enumerate(members):
                tail_at[i] = (off + n * tkey[1] * C, tkey[1])
            off += len(members) * tkey[1] * C
        n = len(chunk)
        clip_f0, clip_m = np.zeros(n, np.int64), np.zeros(n, np.int32)
        tail_off, tail_rows = np.zeros(n, np.int64), np.zeros(n, np.int32)
        skip, valid = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for j, k in enumerate(chunk):
            i, (a, b) = wins[k][0], spans[k]
            fa, fb, tail = self._needs(i, a, b)
            if fb > fa:
                lo, _, first = next(r for r in place[i] if r[0] <= fa and fb <= r[1])
                clip_f0[j], clip_m[j] = first + fa - lo, fb - fa
            if tail:
                tail_off[j], tail_rows[j] = tail_at[i]
            if b > a:                                         # (an empty window of a dense batch: a span of silence)
                skip[j], valid[j] = a - fa * cut, b - a
        on_dev = getattr(br, "clips_window_add", None)
        if on_dev is None:
            out, out_off = clips_window_host(frames, clip_f0, clip_m, N, C, ratio, tails, tail_off, tail_rows, skip, valid, out_format)
            for j, k in enumerate(chunk):
                piece = out[int(out_off[j]):int(out_off[j + 1])]
                if dense is None:
                    finish(k, piece)
                else:
                    dense[k, :len(piece)] = piece
                    dense[k, len(piece):] = from_f64(np.zeros(1), dense.dtype)
            return
        win = None
        if ratio > 1:
            L = N - cut
            win = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))       # Decoder._overlap_host's weights
        if dense is not None:
            on_dev(frames, clip_f0, clip_m, N, C, ratio, tails, tail_off, tail_rows, skip, valid, out_format, win,
                   span=np.full(n, pad_to, np.int64), dst_row=np.asarray(chunk, np.int64) * pad_to, out=dense)
            return
        out, out_off = on_dev(frames, clip_f0, clip_m, N, C, ratio, tails, tail_off, tail_rows, skip, valid, out_format, win,
                              as_tensor=as_tensor)
        step = C * np.dtype(ff_format_to_numpy_type(out_format)).itemsize if as_tensor and out_format is not None else 1
        for j, k in enumerate(chunk):
            finish(k, out[int(out_off[j]) * step:int(out_off[j + 1]) * step])


def decode_windows(streams, windows, *, fix_error: bool = False, bridge=None, **kw) -> WindowResult:
    """``StreamIndex(streams, fix_error=fix_error, bridge=bridge).decode(windows, **kw)``: a throw-away index for one call.  A
    window's stream is its position in ``streams``."""
    return StreamIndex(streams, fix_error=fix_error, bridge=bridge).decode(windows, **kw)
