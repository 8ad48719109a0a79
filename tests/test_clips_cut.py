"""frad_clips_frame_cut alone: the Encoder's frame cut (encoder.py:72-93) for the frames of many clips in one launch.

"emu": the CPU interpreter build of the same kernel source, "gpu": the MI355X.  Both legs call the C-ABI with raw pointers, so
that the guard bytes around `out` are the test's own.  The expected result is numpy slicing; a gather has no tolerance."""
import numpy as np
import pytest

from test_clips_ola import be, Emu, Gpu, _backends  # noqa: F401  (the two backends and their fixture)

GUARD = 64


def expected(src: np.ndarray, row_src, row_valid, row_len, step):
    out = np.zeros((len(row_src), row_len * step), np.uint8)
    for r, (at, n) in enumerate(zip(row_src, row_valid)):
        out[r, :n * step] = src[at * step:(at + n) * step]
    return out


def run(be, src, row_src, row_valid, row_len, step, src_shift=0, out_shift=0):
    """-> the rows; `src_shift` / `out_shift` bytes put the two buffers off their 16-byte alignment"""
    rs, rv = np.ascontiguousarray(row_src, np.int64), np.ascontiguousarray(row_valid, np.int32)
    n, nb = len(rs), len(rs) * row_len * step
    held = np.full(src_shift + src.size + 16, 0x5A, np.uint8)
    held[src_shift:src_shift + src.size] = src
    d_src, d_rs, d_rv = be.put(held), be.put(rs if n else np.zeros(1, np.int64)), be.put(rv if n else np.zeros(1, np.int32))
    d_out = be.put(np.full(GUARD + out_shift + nb + GUARD, 0xA5, np.uint8))
    be.lib.clips_frame_cut(be.ptr(d_src) + src_shift, be.ptr(d_rs), be.ptr(d_rv), n, row_len, step, be.ptr(d_out) + GUARD + out_shift,
                           be.stream)
    raw = be.get(d_out)
    lo = GUARD + out_shift
    assert (raw[:lo] == 0xA5).all() and (raw[lo + nb:] == 0xA5).all(), "guard bytes were written"
    return raw[lo:lo + nb].reshape(n, row_len * step)


def plan(rng, have, row_len, hop, n_rows):
    """rows `hop` sample-frames apart (hop < row_len: they overlap), every edge value of row_valid among them"""
    edge = [0, 1, row_len - 1, row_len]
    rv = np.array([edge[r % 4] if r % 3 == 0 else int(rng.integers(0, row_len + 1)) for r in range(n_rows)], np.int32)
    rs = (np.arange(n_rows, dtype=np.int64) * hop) % max(have - row_len, 1)
    rs[rv == 0] = have                                         # an all-padding row may point at the end of the source
    return rs, rv


# step: 1 = u8 mono, 6 = three channels of s16 (no power of two), 16 = f64 stereo; row lengths whose byte size is (128) and
# is not (50, 3) a multiple of 16 -- at step 1 a row of 3 bytes puts five rows into one 16-byte store; 1 row, and enough rows
# for several blocks' tiles (a tile is 16 KiB of output)
@pytest.mark.parametrize("step", [1, 6, 16])
@pytest.mark.parametrize("row_len", [128, 50, 3])
def test_rows_are_numpy_slices(be, step, row_len):
    rng = np.random.default_rng(step * 1000 + row_len)
    for n_rows in (1, 7, 40000 // (row_len * step) + 37):
        hop = max(row_len // 2, 1)
        have = n_rows * hop + 2 * row_len + 5
        src = rng.integers(1, 256, have * step, dtype=np.uint8)     # no zero byte: padding cannot be mistaken for data
        rs, rv = plan(rng, have, row_len, hop, n_rows)
        want = expected(src, rs, rv, row_len, step)
        for src_shift, out_shift in ((0, 0), (1, 0), (3, 5), (0, 15), (7, 8)):      # source offsets that are odd in bytes too
            got = run(be, src, rs, rv, row_len, step, src_shift, out_shift)
            assert np.array_equal(got, want), (n_rows, src_shift, out_shift)


def test_odd_source_offsets_at_step_one(be):
    rng = np.random.default_rng(5)
    src = rng.integers(1, 256, 4000, dtype=np.uint8)
    rs = np.array([1, 3, 17, 255, 1001, 3871], np.int64)
    rv = np.array([128, 127, 1, 0, 128, 128], np.int32)
    assert np.array_equal(run(be, src, rs, rv, 128, 1), expected(src, rs, rv, 128, 1))


def test_every_row_valid_edge_and_a_full_overlap(be):
    src = np.arange(1, 1 + 60 * 6, dtype=np.int64).astype(np.uint8) | 1
    for row_len in (50, 16):
        rs = np.array([0, 0, 1, 2, 60 - row_len, 60], np.int64)    # rows 0 and 1 are the same sample-frames
        rv = np.array([row_len, row_len, row_len - 1, 1, row_len, 0], np.int32)
        assert np.array_equal(run(be, src, rs, rv, row_len, 6, 0, 2), expected(src, rs, rv, row_len, 6))


def test_zero_rows_write_nothing(be):
    got = run(be, np.ones(64, np.uint8), [], [], 128, 4)
    assert got.shape == (0, 512)


def test_invalid_scalars_are_refused(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    for n_rows, row_len, step in ((1, 128, 0), (1, 128, -1), (1, 0, 4), (1, -5, 4), (-1, 128, 4)):
        with pytest.raises(FradError) as e:
            be.lib.clips_frame_cut(be.ptr(z), be.ptr(z), be.ptr(z), n_rows, row_len, step, be.ptr(z), be.stream)
        assert e.value.status == -1
    with pytest.raises(FradError):
        be.lib.clips_frame_cut(0, be.ptr(z), be.ptr(z), 1, 4, 4, be.ptr(z), be.stream)


@pytest.mark.gpu
def test_core_wrapper_checks_the_offsets_before_it_launches():
    """core.clips_frame_cut: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    step, row_len = 6, 50
    host = np.random.default_rng(1).integers(1, 256, 200 * step + 4, dtype=np.uint8)     # 200 sample-frames and 4 stray bytes
    src = torch.from_numpy(host).to("cuda:0")
    rs, rv = [0, 150, 199, 200], [50, 50, 1, 0]
    out = core.clips_frame_cut(src, rs, rv, row_len, step)
    assert tuple(out.shape) == (4, row_len * step) and np.array_equal(out.cpu().numpy(), expected(host, rs, rv, row_len, step))
    assert tuple(core.clips_frame_cut(src, [], [], row_len, step).shape) == (0, row_len * step)
    for bad in (dict(rs=[151], rv=[50]), dict(rs=[200], rv=[1]), dict(rs=[-1], rv=[1]), dict(rs=[0], rv=[51]), dict(rs=[0], rv=[-1]),
                dict(rs=[0, 1], rv=[1]), dict(row_len=0), dict(step=0), dict(src=src.cpu()), dict(src=src.view(torch.int16)),
                dict(rs=[1 << 62], rv=[1]), dict(rs=[(1 << 63) - 1], rv=[1]), dict(rs=[(1 << 63) - 50], rv=[50])):
        kw = dict(src=src, rs=rs, rv=rv, row_len=row_len, step=step)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            core.clips_frame_cut(kw["src"], kw["rs"], kw["rv"], kw["row_len"], kw["step"])
