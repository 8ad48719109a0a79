"""frad_clips_overlap_add alone: Decoder.overlap + flush() (decoder.py:28-46, 110-114) for many clips in one launch, ragged output.

"emu": the CPU interpreter build of the same kernel source (also the `make emu-asan` build through FRAD_EMU_LIB), "gpu": the
MI355X.  Both legs call the C-ABI with raw pointers, so that the guard bytes behind `out` are the test's own.

Bounds.  Against the per-clip model (oracle OverlapAdd + flush, numpy's cos) the float64 output may differ in the last bits of the
Hann weights, as frad_p1_overlap_add does: 1e-12 * max(1, max|want|), the bound tests/test_parity_p1.py:139 and
tests/test_stream.py:154 use for the same comparison.  Against chaining frad_p1_overlap_add per clip -- the same arithmetic in
the same build -- it is array_equal, and every other output format equals frad_from_f64 of the float64 output byte for byte."""
import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, pcm_dtype_code
from oracle import frad_oracle as fo

INT_FORMATS = ("u8", "u16le", "u16be", "u32le", "u32be", "s8", "s16le", "s16be", "s32le", "s32be", "s64le", "s64be", "u64le")
FLOAT_FORMATS = ("f16le", "f16be", "f32le", "f32be", "f64le", "f64be")
GUARD = 64


class Emu:
    name = "emu"

    def __init__(self):
        from helpers import build_emulator
        from frad_python_amd._lib import FradLib
        self.lib = FradLib(build_emulator())

    def put(self, a):
        return np.ascontiguousarray(a)

    def ptr(self, a):
        return a.ctypes.data if a is not None else 0

    def get(self, a):
        return a

    stream = 0


class Gpu:
    name = "gpu"

    def __init__(self):
        import torch
        from frad_python_amd import _lib
        self.t, self.lib = torch, _lib.load()

    def put(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def ptr(self, a):
        return a.data_ptr() if a is not None else 0

    def get(self, a):
        self.t.cuda.synchronize()
        return a.cpu().numpy()

    @property
    def stream(self):
        return int(self.t.cuda.current_stream().cuda_stream)


_backends = {}


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param not in _backends:
        _backends[request.param] = Emu() if request.param == "emu" else Gpu()
    return _backends[request.param]


def hann(L):
    return 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))


def layout(clips, N, C, ratio):
    """clips: [(frames [m, N, C], tail [rows, C] or None)] -> the kernel's arrays"""
    cut = N * (ratio - 1) // ratio if ratio else N
    L = N - cut
    frames = np.concatenate([c[0] for c in clips]) if clips else np.zeros((0, N, C))
    cf = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([len(c[0]) for c in clips], out=cf[1:])
    tail_rows = np.array([0 if c[1] is None else len(c[1]) for c in clips], np.int32)
    tails = [c[1].reshape(-1) for c in clips if c[1] is not None]
    tail_off = np.zeros(len(clips), np.int64)
    at = 7                                                     # the last frames need not start the buffer
    for j, c in enumerate(clips):
        if c[1] is not None:
            tail_off[j] = at
            at += c[1].size
    flat = np.concatenate([np.full(7, np.nan)] + tails + [np.full(5, np.nan)])
    rows = [len(c[0]) * cut + (len(c[1]) if c[1] is not None else (L if len(c[0]) else 0)) for c in clips]
    out_off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum(rows, out=out_off[1:])
    return frames, cf, flat, tail_off, tail_rows, out_off


def run(be, clips, N, C, ratio, fmt="f64le", flags=2, win=True, misalign=0):
    frames, cf, flat, tail_off, tail_rows, out_off = layout(clips, N, C, ratio)
    dt = ff_format_to_numpy_type(fmt)
    total = int(out_off[-1])
    nb = total * C * dt.itemsize
    cut = N * (ratio - 1) // ratio if ratio else N
    d_frames = be.put(frames) if frames.size else None
    d_cf, d_flat, d_to, d_tr, d_oo = be.put(cf), be.put(flat), be.put(tail_off), be.put(tail_rows), be.put(out_off)
    d_win = be.put(hann(N - cut)) if win and ratio and N - cut else None
    d_out = be.put(np.full(misalign + nb + GUARD, 0xA5, np.uint8))
    be.lib.clips_overlap_add(be.ptr(d_frames), be.ptr(d_cf), len(clips), N, C, ratio, be.ptr(d_flat), be.ptr(d_to), be.ptr(d_tr),
                             be.ptr(d_win), pcm_dtype_code(fmt), be.ptr(d_out) + misalign, be.ptr(d_oo), total, be.stream, flags)
    raw = be.get(d_out)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    return np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(total, C), out_off


def model(clips, ratio):
    out = []
    for frames, tail in clips:
        ola = fo.OverlapAdd()
        pieces = [ola.push(f.copy(), True, ratio) for f in frames]
        if tail is not None:
            pieces.append(ola.push(tail.copy(), True, ratio))
        pieces.append(ola.flush().reshape(-1, frames.shape[2]))
        out.append(np.concatenate([p for p in pieces if p.size] or [np.zeros((0, frames.shape[2]))]))
    return out


def chained(be, clips, N, C, ratio):
    """frad_p1_overlap_add per clip: [m * cut, C] followed by the returned tail (defined for ratio >= 2, m >= 1)"""
    cut = N * (ratio - 1) // ratio
    res = []
    for frames, _ in clips:
        m = len(frames)
        if m == 0:
            res.append(None)
            continue
        d_f, d_o, d_t = be.put(frames), be.put(np.zeros((m, cut, C))), be.put(np.zeros((N - cut, C)))
        be.lib.p1_overlap_add(be.ptr(d_f), m, N, C, ratio, 0, be.ptr(d_o), be.ptr(d_t), be.stream)
        res.append((be.get(d_o).reshape(-1, C).copy(), be.get(d_t).copy()))
    return res


def make_clips(rng, N, C, ratio, ms, tails):
    cut = N * (ratio - 1) // ratio if ratio else N
    L = N - cut
    rows_of = {"none": None, "L": max(L, 1), "L+1": L + 1, "N-1": N - 1, "long": N + 37}
    clips = []
    for m in ms:
        for t in tails:
            rows = rows_of[t]
            clips.append((rng.uniform(-1.1, 1.1, (m, N, C)), None if rows is None else rng.uniform(-1.1, 1.1, (rows, C))))
    return clips


@pytest.mark.parametrize("N", [128, 2048, 2240])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_against_the_per_clip_model_and_the_chained_kernel(be, N, C):
    rng = np.random.default_rng(N * 10 + C)
    for ratio in (0, 2, 3, 16, 256):
        clips = make_clips(rng, N, C, ratio, (0, 1, 2, 7), ("none", "L", "L+1", "N-1", "long"))
        order = rng.permutation(len(clips))
        clips = [clips[i] for i in order]
        got, out_off = run(be, clips, N, C, ratio)
        want = model(clips, ratio)
        cut = N * (ratio - 1) // ratio if ratio else N
        ref = chained(be, clips, N, C, ratio) if ratio >= 2 else None
        for j, w in enumerate(want):
            g = got[out_off[j]:out_off[j + 1]]
            assert g.shape == w.shape, (ratio, j)
            if not w.size:
                continue
            err = np.max(np.abs(g - w))
            assert err <= 1e-12 * max(1.0, np.max(np.abs(w))), (ratio, j, err)
            if ratio == 0:
                assert np.array_equal(g, w)                    # a plain gather
            elif ref[j] is not None:
                m = len(clips[j][0])
                assert np.array_equal(g[:m * cut], ref[j][0]), (ratio, j)
                if clips[j][1] is None:
                    assert np.array_equal(g[m * cut:], ref[j][1]), (ratio, j)
        # the last frames the Decoder fades on the host take the caller's window: with it they ARE the model's numbers
        if ratio >= 2:
            L = N - cut
            for j, (frames, tail) in enumerate(clips):
                if tail is not None and len(frames) and len(tail) - len(tail) * (ratio - 1) // ratio != L:
                    m = len(frames)
                    assert np.array_equal(got[out_off[j] + m * cut:out_off[j + 1]], want[j][m * cut:]), (ratio, j)


@pytest.mark.parametrize("flags", [2, 0])
@pytest.mark.parametrize("fmt", INT_FORMATS + FLOAT_FORMATS)
def test_every_output_format_is_from_f64_of_the_float64_output(be, fmt, flags):
    rng = np.random.default_rng(11)
    N, C, ratio = 128, 3, 16
    clips = make_clips(rng, N, C, ratio, (0, 1, 2, 7), ("none", "L", "N-1", "long"))
    f64, off = run(be, clips, N, C, ratio)
    for misalign in (0, 2 * ff_format_to_numpy_type(fmt).itemsize):
        got, off2 = run(be, clips, N, C, ratio, fmt, flags, misalign=misalign)
        assert np.array_equal(off, off2)
        dt = ff_format_to_numpy_type(fmt)
        src = be.put(f64)
        dst = be.put(np.zeros(f64.size * dt.itemsize + 16, np.uint8))
        be.lib.from_f64(be.ptr(src), f64.size, pcm_dtype_code(fmt), be.ptr(dst), be.stream, flags)
        want = be.get(dst)[:f64.size * dt.itemsize]
        assert got.tobytes() == want.tobytes(), (fmt, flags, misalign)


def test_empty_clips_and_window_less_call(be):
    rng = np.random.default_rng(3)
    N, C, ratio = 128, 2, 16
    empty = (np.zeros((0, N, C)), None)
    clips = [empty, empty] + make_clips(rng, N, C, ratio, (2,), ("none", "N-1")) + [empty] + make_clips(rng, N, C, ratio, (1,), ("L",)) + [empty]
    want = model(clips, ratio)
    for win in (True, False):
        got, off = run(be, clips, N, C, ratio, win=win)
        for j, w in enumerate(want):
            g = got[off[j]:off[j + 1]]
            assert g.shape == w.shape and (not w.size or np.max(np.abs(g - w)) <= 1e-12 * max(1.0, np.max(np.abs(w))))
    got, off = run(be, [empty, empty], N, C, ratio)
    assert got.shape == (0, C)


def test_host_checkable_arguments_are_refused(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    for (N, C, ratio, code) in ((0, 2, 16, 22), (128, 0, 16, 22), (128, 2, 1, 22), (128, 2, 257, 22), (128, 2, -1, 22), (128, 2, 16, 16), (128, 2, 16, 24)):
        with pytest.raises(FradError):
            be.lib.clips_overlap_add(be.ptr(z), be.ptr(z), 1, N, C, ratio, be.ptr(z), be.ptr(z), be.ptr(z), 0, code, be.ptr(z), be.ptr(z), 1, be.stream)


@pytest.mark.gpu
def test_core_wrapper_checks_the_index_arrays_before_it_launches():
    """core.clips_overlap_add: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    N, C, ratio = 128, 2, 16
    L = N - N * (ratio - 1) // ratio
    frames = torch.zeros((3, N, C), dtype=torch.float64, device="cuda:0")
    tails = torch.zeros(40 * C, dtype=torch.float64, device="cuda:0")
    out, off = core.clips_overlap_add(frames, [0, 2, 3], N, C, ratio, tails, [0, 0], [0, 40])
    assert off.tolist() == [0, 2 * 120 + L, 2 * 120 + L + 120 + 40] and tuple(out.shape) == (off[-1], C)
    for bad in (dict(clip_frame0=[0, 2, 4]), dict(clip_frame0=[1, 2, 3]), dict(clip_frame0=[0, 3, 2]), dict(tail_rows=[0, L - 1]),
                dict(tail_rows=[0, 41]), dict(tail_off=[0, 1]), dict(tail_off=[0, -1]), dict(ratio=1), dict(ratio=300), dict(C=3),
                dict(tail_win=np.zeros(L + 1)), dict(tail_rows=[0]), dict(frames=frames.cpu())):
        kw = dict(frames=frames, clip_frame0=[0, 2, 3], N=N, C=C, ratio=ratio, tails=tails, tail_off=[0, 0], tail_rows=[0, 40], tail_win=None)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            core.clips_overlap_add(kw["frames"], kw["clip_frame0"], kw["N"], kw["C"], kw["ratio"], kw["tails"], kw["tail_off"], kw["tail_rows"],
                                   None, kw["tail_win"])
    with pytest.raises(ValueError):
        core.clips_overlap_add(frames, [0, 2, 3], N, C, ratio, tails, [0, 0], [0, 40], "s17le")
