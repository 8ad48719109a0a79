"""frad_clips_carry_add alone: frad_p1_overlap_add_pcm for many live streams in one launch -- every clip starts from the fragment
its stream carried in and ends in the fragment it carries out.

Legs, raw pointers and guard bytes as in test_clips_window.py ("emu": the CPU interpreter build of the same kernel source, "gpu":
the MI355X); the backends and helpers are test_clips_ola.py's.  The fragments read lie in one buffer with NaNs between them, the
fragments written in another that is NaN throughout before the launch, so a read or a write beside a fragment shows.

Bounds.  Against frad_p1_overlap_add_pcm (and frad_clips_overlap_add) of the same build the bytes are equal: the same
operations on the same numbers in the same order.  Against the numpy model ``pool.clips_carry_host`` the float64 output may
differ in the last bits of the Hann weights: 1e-12 * max(1, max|want|), the bound test_clips_ola.py documents for the same
comparison; the other formats are compared after ``from_f64`` of the kernel's own float64 output."""
import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64, pcm_dtype_code
from frad_python_amd.pool import clips_carry_host
from test_clips_ola import GUARD, be, run as run_ola  # noqa: F401  (be: the fixture)

FORMATS = ("f64le", "s16le", "u8", "f32be")
GEOMETRIES = [(128, 3, 16), (128, 2, 2), (128, 1, 0), (2240, 2, 3)]
GAP = 3                                                        # NaNs between two fragments


def geometry(N, ratio):
    cut = N * (ratio - 1) // ratio if ratio else N
    return cut, N - cut


def make_clips(rng, N, C, ratio, ms=(0, 1, 2, 7)):
    """[(frames [m, N, C], fragment [L, C] or None)]: every m with and without a fragment, shuffled"""
    L = geometry(N, ratio)[1]
    clips = [(rng.uniform(-1.1, 1.1, (m, N, C)), rng.uniform(-1.1, 1.1, (L, C)) if has else None) for m in ms for has in (True, False)]
    return [clips[i] for i in rng.permutation(len(clips))]


def launch(be, frames, cf, N, C, ratio, prev_ptrs, next_ptrs, fmt, d_out, out_at, out_off, out_rows, flags=2):
    """The raw entry point on device arrays; the pointer tables are host lists (None: a null table)"""
    d_frames = be.put(frames) if frames is not None and frames.size else None
    d_cf, d_off = be.put(np.ascontiguousarray(cf, np.int64)), be.put(np.ascontiguousarray(out_off, np.int64))
    d_pp = be.put(np.array(prev_ptrs, np.uint64)) if prev_ptrs is not None else None
    d_np = be.put(np.array(next_ptrs, np.uint64)) if next_ptrs is not None else None
    be.lib.clips_carry_add(be.ptr(d_frames), be.ptr(d_cf), len(cf) - 1, N, C, ratio, be.ptr(d_pp), be.ptr(d_np), pcm_dtype_code(fmt), flags,
                           be.ptr(d_out) + out_at, be.ptr(d_off), out_rows, be.stream)
    be.get(d_cf)                                               # (the launch has ended before its tables go)


def run(be, clips, N, C, ratio, fmt="f64le", misalign=0, carry=True, flags=2):
    """-> (out [rows, C], out_off, next fragments per clip or None).  Checks the guards behind ``out``, that the fragments read
    are unchanged, and that nothing but the named fragments is written: the slot of a clip without a frame stays NaN."""
    cut, L = geometry(N, ratio)
    frames = np.concatenate([c[0] for c in clips]) if clips else np.zeros((0, N, C))
    cf = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([len(c[0]) for c in clips], out=cf[1:])
    out_off = cf * cut
    dt = ff_format_to_numpy_type(fmt)
    total = int(out_off[-1])
    nb = total * C * dt.itemsize
    slot = L * C + GAP
    flat_prev = np.full(GAP + len(clips) * slot, np.nan)
    for j, c in enumerate(clips):
        if c[1] is not None and L:
            flat_prev[GAP + j * slot:GAP + j * slot + L * C] = c[1].reshape(-1)
    d_prev, d_next = be.put(flat_prev.copy()), be.put(np.full(GAP + len(clips) * slot, np.nan))
    at = lambda d, j: be.ptr(d) + 8 * (GAP + j * slot)
    prev_ptrs = [at(d_prev, j) if c[1] is not None and L else 0 for j, c in enumerate(clips)]
    next_ptrs = [at(d_next, j) for j in range(len(clips))] if carry else None
    d_out = be.put(np.full(misalign + nb + GUARD, 0xA5, np.uint8))
    launch(be, frames, cf, N, C, ratio, prev_ptrs, next_ptrs, fmt, d_out, misalign, out_off, total, flags)
    raw = be.get(d_out)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    assert be.get(d_prev).tobytes() == flat_prev.tobytes(), "a fragment that is read was written"
    got_next = be.get(d_next)
    nxt, written = [], np.zeros(got_next.size, bool)
    for j, c in enumerate(clips):
        if carry and L and len(c[0]):
            written[GAP + j * slot:GAP + j * slot + L * C] = True
            nxt.append(got_next[GAP + j * slot:GAP + j * slot + L * C].reshape(L, C).copy())
        else:
            nxt.append(None)
    assert np.isnan(got_next[~written]).all(), "something beside the named fragments was written"
    out = np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(total, C)
    if fmt == "f64le":
        assert np.isfinite(out).all() and all(np.isfinite(x).all() for x in nxt if x is not None), "a NaN between the fragments was read"
    return out, out_off, nxt


def ola_pcm(be, frames, N, C, ratio, prev, fmt):
    """frad_p1_overlap_add_pcm of one stream's frames -> (out [m * cut, C], next_tail)"""
    cut, L = geometry(N, ratio)
    m, dt = len(frames), ff_format_to_numpy_type(fmt)
    d_f, d_t = be.put(frames), be.put(np.zeros((L, C)))
    d_p = be.put(prev) if prev is not None else None
    d_o = be.put(np.zeros(m * cut * C * dt.itemsize + 16, np.uint8))
    be.lib.p1_overlap_add_pcm(be.ptr(d_f), m, N, C, ratio, be.ptr(d_p), pcm_dtype_code(fmt), be.ptr(d_o), be.ptr(d_t), be.stream)
    return np.frombuffer(be.get(d_o)[:m * cut * C * dt.itemsize].tobytes(), dt).reshape(m * cut, C), be.get(d_t).copy()


# ------------------------------------------------------------------------------------ 1. frad_p1_overlap_add_pcm, clip by clip
@pytest.mark.parametrize("N,C,ratio", GEOMETRIES)
def test_every_clip_is_frad_p1_overlap_add_pcm_byte_for_byte(be, N, C, ratio):
    rng = np.random.default_rng(N + 7 * C + ratio)
    clips = make_clips(rng, N, C, ratio)
    cut, L = geometry(N, ratio)
    for fmt in FORMATS:
        dt = ff_format_to_numpy_type(fmt)
        for misalign in (0, 2 * dt.itemsize):
            got, off, nxt = run(be, clips, N, C, ratio, fmt, misalign)
            assert off.tolist() == np.cumsum([0] + [len(c[0]) * cut for c in clips]).tolist()
            for j, (frames, prev) in enumerate(clips):
                g = got[off[j]:off[j + 1]]
                if not len(frames):
                    assert g.size == 0 and nxt[j] is None
                elif ratio:
                    want, tail = ola_pcm(be, frames, N, C, ratio, prev, fmt)
                    assert g.tobytes() == want.tobytes(), (fmt, misalign, j)
                    assert nxt[j].tobytes() == tail.tobytes() == frames[-1, cut:].tobytes(), (fmt, misalign, j)
                else:                                          # no overlap: a gather and the conversion
                    src = be.put(frames)
                    dst = be.put(np.zeros(frames.size * dt.itemsize + 16, np.uint8))
                    be.lib.from_f64(be.ptr(src), frames.size, pcm_dtype_code(fmt), be.ptr(dst), be.stream, 2)
                    assert g.tobytes() == be.get(dst)[:frames.size * dt.itemsize].tobytes(), (fmt, misalign, j)
                    assert nxt[j] is None


# --------------------------------------------------------------------------------------------- 2. frad_clips_overlap_add
@pytest.mark.parametrize("N,C,ratio", GEOMETRIES)
def test_a_clip_without_a_fragment_is_the_head_of_frad_clips_overlap_add(be, N, C, ratio):
    rng = np.random.default_rng(3 * N + C + ratio)
    cut, L = geometry(N, ratio)
    clips = [(c[0], None) for c in make_clips(rng, N, C, ratio)]
    for fmt in FORMATS:
        got, off, nxt = run(be, clips, N, C, ratio, fmt)
        whole, woff = run_ola(be, clips, N, C, ratio, fmt)
        f64, _ = run_ola(be, clips, N, C, ratio)
        for j, (frames, _) in enumerate(clips):
            m = len(frames)
            assert got[off[j]:off[j + 1]].tobytes() == whole[woff[j]:woff[j] + m * cut].tobytes(), (fmt, j)
            if m and L:
                assert nxt[j].tobytes() == f64[woff[j] + m * cut:woff[j + 1]].tobytes(), (fmt, j)      # the flush rows, float64


# ------------------------------------------------------------------------------------------------------ 3. split invariance
@pytest.mark.parametrize("N,C,ratio", GEOMETRIES)
def test_three_launches_with_the_fragment_carried_give_the_bytes_of_one(be, N, C, ratio):
    rng = np.random.default_rng(N + C + 5 * ratio)
    cut, L = geometry(N, ratio)
    clips = [(rng.uniform(-1.1, 1.1, (7, N, C)), rng.uniform(-1.1, 1.1, (L, C)) if has else None) for has in (True, False, True)]
    for fmt in FORMATS:
        dt = ff_format_to_numpy_type(fmt)
        one, off, last = run(be, clips, N, C, ratio, fmt)
        # 3 + 0 + 4 frames; the fragments alternate between two buffers, the empty launch leaves the pending one pending
        n, per = len(clips), max(L * C, 1)
        first = np.full((n, per), np.nan)
        for j, c in enumerate(clips):
            if c[1] is not None and L:
                first[j] = c[1].reshape(-1)
        bufs = [be.put(first), be.put(np.full((n, per), np.nan))]
        ptrs = lambda d: [be.ptr(d) + 8 * per * j for j in range(n)]
        live = [ptrs(bufs[0])[j] if c[1] is not None and L else 0 for j, c in enumerate(clips)]
        pieces, cur = [[] for _ in clips], 0
        for lo, hi in ((0, 3), (3, 3), (3, 7)):
            frames = np.concatenate([c[0][lo:hi] for c in clips])
            cf = np.arange(n + 1) * (hi - lo)
            rows = int(cf[-1]) * cut
            d_out = be.put(np.full(rows * C * dt.itemsize + GUARD, 0xA5, np.uint8))
            before = be.get(bufs[1 - cur]).tobytes()
            launch(be, frames, cf, N, C, ratio, live, ptrs(bufs[1 - cur]), fmt, d_out, 0, cf * cut, rows)
            raw = be.get(d_out)
            assert (raw[rows * C * dt.itemsize:] == 0xA5).all()
            for j in range(n):
                pieces[j].append(raw[int(cf[j]) * cut * C * dt.itemsize:int(cf[j + 1]) * cut * C * dt.itemsize])
            if hi > lo:
                if L:
                    live = ptrs(bufs[1 - cur])
                cur = 1 - cur
            elif L:
                assert be.get(bufs[1 - cur]).tobytes() == before, "an empty clip's next buffer was written"
        for j in range(n):
            assert np.concatenate(pieces[j]).tobytes() == one[off[j]:off[j + 1]].tobytes(), (fmt, j)
            if L:
                assert be.get(bufs[cur])[j].tobytes() == last[j].tobytes(), (fmt, j)


# --------------------------------------------------------------------------------------------------------- 4. the numpy model
@pytest.mark.parametrize("N,C,ratio", GEOMETRIES)
def test_against_the_numpy_model(be, N, C, ratio):
    rng = np.random.default_rng(11 * N + C + ratio)
    clips = make_clips(rng, N, C, ratio)
    frames = np.concatenate([c[0] for c in clips])
    cf = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([len(c[0]) for c in clips], out=cf[1:])
    want, woff, wnext = clips_carry_host(frames, cf, N, C, ratio, [c[1] for c in clips])
    f64, off, nxt = run(be, clips, N, C, ratio)
    assert np.array_equal(off, woff) and f64.shape == want.shape
    err = np.max(np.abs(f64 - want))
    print(f"[model] N={N} C={C} ratio={ratio}: max|got - want| = {err:.3e}")
    assert err <= 1e-12 * max(1.0, np.max(np.abs(want)))
    L = geometry(N, ratio)[1]
    for j, c in enumerate(clips):
        if len(c[0]) and L:
            assert np.array_equal(nxt[j], wnext[j]), j         # a copy on both sides
        elif L:
            assert nxt[j] is None and (wnext[j] is c[1] or wnext[j] is None)
        else:
            assert nxt[j] is None and wnext[j] is None
    for fmt in FORMATS[1:]:
        got, _, _ = run(be, clips, N, C, ratio, fmt)
        assert got.tobytes() == from_f64(f64, fmt).astype(ff_format_to_numpy_type(fmt)).tobytes(), fmt
    assert clips_carry_host(frames, cf, N, C, ratio, None, "s16le")[0].dtype == np.dtype("<i2")


# ------------------------------------------------------------------------------------------------- 5. null tables, bounds
def test_null_tables_and_a_short_out_rows(be):
    rng = np.random.default_rng(5)
    N, C, ratio = 128, 2, 16
    cut, L = geometry(N, ratio)
    clips = make_clips(rng, N, C, ratio)
    want, off, _ = run(be, clips, N, C, ratio)
    got, _, nxt = run(be, clips, N, C, ratio, carry=False)     # next_ptr NULL: nothing is carried, the rows are the same
    assert got.tobytes() == want.tobytes() and all(x is None for x in nxt)
    bare = [(c[0], None) for c in clips]
    frames = np.concatenate([c[0] for c in bare])
    cf = np.zeros(len(bare) + 1, np.int64)
    np.cumsum([len(c[0]) for c in bare], out=cf[1:])
    want, off, _ = run(be, bare, N, C, ratio)
    for rows, first in ((int(off[-1]) - 77, 0), (int(off[-1]), 5)):
        # out_rows below out_off[n_clips]: nothing beyond it is written; out_off[0] > 0: the rows before it are left alone
        d_out = be.put(np.full(int(off[-1] + first) * C * 8 + GUARD, 0xA5, np.uint8))
        launch(be, frames, cf, N, C, ratio, None, None, "f64le", d_out, 0, off + first, rows + first)
        raw = be.get(d_out)
        lo, hi = first * C * 8, (rows + first) * C * 8
        assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all()
        assert raw[lo:hi].tobytes() == want.tobytes()[:hi - lo]


# ---------------------------------------------------------------------------------------------------------- 6. status codes
def test_status_codes(be):
    from frad_python_amd._lib import FradError
    N, C, ratio = 16, 2, 4
    cut, L = geometry(N, ratio)
    frames = be.put(np.ones((1, N, C)))
    cf, off = be.put(np.array([0, 1], np.int64)), be.put(np.array([0, cut], np.int64))
    frag = be.put(np.full((2, L, C), 7.0))
    pp, np_ = be.put(np.array([be.ptr(frag)], np.uint64)), be.put(np.array([be.ptr(frag) + 8 * L * C], np.uint64))
    out = be.put(np.full(cut * C * 8 + GUARD, 0xA5, np.uint8))
    args = lambda N=N, C=C, ratio=ratio, code=22, n=1, rows=cut, **nul: (
        nul.get("frames", be.ptr(frames)), nul.get("clip_frame0", be.ptr(cf)), n, N, C, ratio, be.ptr(pp), be.ptr(np_), code, 2,
        nul.get("out", be.ptr(out)), nul.get("out_off", be.ptr(off)), rows, be.stream)
    for bad in (dict(N=0), dict(C=0), dict(ratio=1), dict(ratio=257), dict(ratio=-1), dict(code=16), dict(code=24), dict(n=-1), dict(rows=-1),
                dict(N=1, ratio=2), dict(frames=0), dict(clip_frame0=0), dict(out=0), dict(out_off=0)):
        with pytest.raises(FradError) as e:
            be.lib.clips_carry_add(*args(**bad))
        assert e.value.status == -1, bad                       # FRAD_E_INVALID
        assert (be.get(out) == 0xA5).all() and (be.get(frag) == 7.0).all(), bad
    assert be.lib.clips_carry_add(*([0] * 13)) is None         # the all-zero call (tests/test_abi.py makes it for every entry point)
    assert be.lib.clips_carry_add(*args(n=0, N=0, frames=0, out=0)) is None        # no clip: nothing is looked at
    assert be.lib.clips_carry_add(*args(rows=0, frames=0, out=0)) is None
    assert (be.get(out) == 0xA5).all() and (be.get(frag) == 7.0).all()
    assert be.lib.clips_carry_add(*args()) is None
    raw = be.get(out)
    assert (raw[cut * C * 8:] == 0xA5).all() and (be.get(frag)[1] == 1.0).all() and (be.get(frag)[0] == 7.0).all()


@pytest.mark.gpu
def test_core_wrapper_checks_the_tables_before_it_launches():
    """core.clips_carry_add: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    N, C, ratio = 16, 2, 4
    cut, L = geometry(N, ratio)
    dev = "cuda:0"
    frames = torch.rand((3, N, C), dtype=torch.float64, device=dev)
    a, b = torch.rand((2, L, C), dtype=torch.float64, device=dev), torch.full((2, L, C), 9.0, dtype=torch.float64, device=dev)
    good = dict(frames=frames, cf=[0, 2, 3], ratio=ratio, prev=[a[0], None], nxt=[b[0], b[1]], fmt=None, out=None)
    run_ = lambda kw: core.clips_carry_add(kw["frames"], kw["cf"], kw.get("N", N), kw.get("C", C), kw["ratio"], kw["prev"], kw["nxt"], kw["fmt"], kw["out"])
    out, off = run_(good)
    assert off.tolist() == [0, 2 * cut, 3 * cut] and tuple(out.shape) == (3 * cut, C)
    assert torch.equal(b[0], frames[1, cut:]) and torch.equal(b[1], frames[2, cut:])
    want, tail = core.p1_overlap_add(frames[:2], ratio, a[0])
    assert torch.equal(out[:2 * cut], want.reshape(-1, C)) and torch.equal(tail, b[0])
    given = torch.zeros((3 * cut + 2, C), dtype=torch.float64, device=dev)
    assert run_(dict(good, out=given))[0] is given and torch.equal(given[:3 * cut], out) and not given[3 * cut:].any()
    raw = torch.zeros(3 * cut * C * 2, dtype=torch.uint8, device=dev)
    assert run_(dict(good, fmt="s16le", out=raw))[0] is raw
    b.fill_(9.0)
    for bad in (dict(frames=frames.cpu()), dict(frames=frames.float()), dict(frames=frames.transpose(1, 2)), dict(cf=[0, 2, 4]),
                dict(cf=[0, 3, 2]), dict(cf=[-1, 2, 3]), dict(cf=[]), dict(ratio=1), dict(ratio=300), dict(C=3), dict(N=1, ratio=2),
                dict(prev=[a[0]]), dict(nxt=[b[0]]), dict(prev=[a[0].float(), None]), dict(prev=[a.reshape(-1), None]),
                dict(prev=[a[0].cpu(), None]), dict(nxt=[a[0], b[1]]), dict(prev=[a[0], None], nxt=[b[0], a[0]]),
                dict(fmt="s17le"), dict(out=given[:3 * cut - 1]), dict(out=raw), dict(fmt="s16le", out=given), dict(fmt="s16le", out=raw[:-2]),
                dict(out=given.cpu())):
        with pytest.raises(ValueError):
            run_(dict(good, **bad))
    torch.cuda.synchronize()
    assert (b == 9.0).all(), "a refused call wrote a fragment"
