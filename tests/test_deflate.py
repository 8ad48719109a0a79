"""Raw DEFLATE deflate on the device (frad_deflate_raw, core.deflate_batch) and ``Encoder(device_deflate=True)``.

The kernel must write zlib's exact bytes: ``zlib.compressobj(-1, zlib.DEFLATED, -15)`` (``compress(body) + flush()``), the
deflate of profile1.py:50 / profile2.py:54.  It is checked on the CPU emulator (``emu``, the same kernel source) and on the
MI355X (``gpu``) against the runtime zlib and against the deflated bytes the golden fixtures hold.  End to end (GPU): the
encoder's streams with the device deflate must be byte-identical to the default path's."""
import os
import zlib

import numpy as np
import pytest

from helpers import build_emulator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 65274                                                  # wsize + MAX_DIST


def _zlib(body: bytes) -> bytes:
    c = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, -15)
    return c.compress(body) + c.flush()


# ------------------------------------------------------------------------------------------------------------- backends
class EmuDeflate:
    def __init__(self):
        from frad_python_amd._lib import FradLib
        self.lib = FradLib(build_emulator())

    def __call__(self, bodies, stride=None, guard=64):
        """-> [(status, bytes)], the destination bytes outside the rows (must stay 0xAB), the rows"""
        n = len(bodies)
        if stride is None:
            stride = self.lib.deflate_stride(max([len(b) for b in bodies] + [0]))
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in bodies], out=off[1:])
        joined = b"".join(bodies)                              # exactly the body bytes: no slack to hide an over-read
        src = np.frombuffer(joined, np.uint8).copy() if joined else np.zeros(1, np.uint8)
        dst = np.full(n * stride + guard + 16, 0xAB, np.uint8)
        base = (-dst.ctypes.data) % 16
        nb = np.zeros(max(n, 1), np.int64)
        st = np.zeros(max(n, 1), np.int32)
        self.lib.deflate_raw(src.ctypes.data, off.ctypes.data, n, dst.ctypes.data + base, stride, nb.ctypes.data, st.ctypes.data)
        rows = dst[base:base + n * stride]
        out = [(int(st[i]), rows[i * stride:i * stride + nb[i]].tobytes()) for i in range(n)]
        return out, np.concatenate([dst[:base], dst[base + n * stride:]]), rows.reshape(n, stride), nb[:n]


class GpuDeflate:
    def __init__(self):
        import torch
        from frad_python_amd import core
        self.torch, self.core = torch, core

    def __call__(self, bodies, stride=None, guard=64):
        t = self.torch
        off = np.zeros(len(bodies) + 1, np.int64)
        np.cumsum([len(b) for b in bodies], out=off[1:])
        src = t.from_numpy(np.frombuffer(b"".join(bodies) + b"\0", np.uint8).copy()).cuda()[:int(off[-1])]
        dst, nb, st = self.core.deflate_batch(src, t.from_numpy(off).cuda())
        rows, nb, st = dst.cpu().numpy(), nb.cpu().numpy(), st.cpu().numpy()
        return [(int(st[i]), rows[i, :nb[i]].tobytes()) for i in range(len(bodies))], None, rows, nb


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def deflate(request):
    return EmuDeflate() if request.param == "emu" else GpuDeflate()


# --------------------------------------------------------------------------------------------------------------- corpus
def _stream_payloads(s: bytes) -> list:
    from frad_python_amd.tools.asfh import ASFH
    pos, out = 0, []
    while pos < len(s):
        a = ASFH()
        a.read(bytes(s[pos:pos + 40]))
        pos += a.header_bytes
        if a.frmbytes and a.profile in (1, 2):
            out.append(bytes(s[pos:pos + a.frmbytes]))
        pos += a.frmbytes
    return out


def _fixture_payloads() -> list:
    """deflated bytes the fixtures hold, written by the reference's zlib: g4 *_frad, the frames of the g3 / g7 / g8 streams"""
    out = []
    g4 = np.load(f"{GOLDEN}/g4_p1.npz")
    out += [g4[k].tobytes() for k in g4.files if k.endswith("_frad")]
    g3 = np.load(f"{GOLDEN}/g3_p1_streams.npz")
    for k in g3.files:
        if k.endswith("_stream"):
            out += _stream_payloads(g3[k].tobytes())
    for name in ("g7_p2", "g8_p2_enc"):
        g = np.load(f"{GOLDEN}/{name}.npz")
        off = g["stream_off"]
        for i in range(len(off) - 1):
            out += _stream_payloads(g["stream"][off[i]:off[i + 1]].tobytes())
    return out


def _fixture_bodies() -> list:
    """pre-deflate bodies: the inflated fixture payloads, g6's Golomb bytes and g8's bodies"""
    out = [zlib.decompress(p, wbits=-15) for p in _fixture_payloads()]
    g6 = np.load(f"{GOLDEN}/g6_p1_more.npz")
    out += [g6[k].tobytes() for k in g6.files if k.endswith("_gol") or (k.startswith("gol_") and k.endswith("_bytes"))]
    g8 = np.load(f"{GOLDEN}/g8_p2_enc.npz")
    off = g8["body_off"]
    out += [g8["body"][off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
    return out


def _edge_bodies() -> list:
    rng = np.random.default_rng(2026)
    r = lambda n, hi=256: rng.integers(0, hi, n, dtype=np.uint8).tobytes()
    out = [b"", b"\x00", b"ab", b"abc", b"abcd", b"aaaa", b"abcabc"]
    out += [r(n) for n in (5, 100, 3000, 20000)]                 # random bytes: stored blocks
    out += [bytes(n) for n in (10, 300, 5000, 40000)]            # all zeros: long matches, the nice cut-off
    out += [(b"xy" * 9000), (b"abc" * 7000), (b"0123456" * 4000)]   # short periods
    out += [r(n, 4) for n in (17000, 40000, 65000)]             # >= 16 383 symbols: once and several times
    out += [r(n, 2) for n in (33000,)]
    # length-3 matches just above and below TOO_FAR (4 096) back
    for d in (4094, 4095, 4096, 4097, 4098):
        pre = b"Q#z" + r(d - 3, 16) + b"Q#z" + r(50, 16)
        out.append(pre)
    # matches at distances around MAX_DIST (32 506) in a body of about 40 KB: as the chain head, and as a later link
    for d in (32505, 32506, 32507):
        key = b"MAXDIST-key!"
        filler = bytes((i * 7 + (i >> 8)) & 0xFF for i in range(d - len(key)))
        head = key + filler + key + r(40000 - d - len(key), 200)
        out.append(head)
        link = key[:5] + filler[:d - 5] + key[:5] + b"#" + key[:4] + r(40000 - d - 15, 200)
        out.append(b"zz" + link)
    # hash collisions at the start of a chain: equal 15-bit hashes, different bytes (the top bits of b[p] drop out)
    col = []
    for k in range(200):
        a = k % 8
        col.append(bytes([(a << 5) | 3, 7, 9]) + bytes([k & 255]))
    out.append(b"".join(col) * 3)
    # literal frequencies on a Fibonacci curve: Huffman lengths past 15 (gen_bitlen's overflow fix)
    fib, a, b = [], 1, 1
    for s in range(25):
        fib.append(a)
        a, b = b, a + b
    lits = np.concatenate([np.full(min(f, 6000), s, np.uint8) for s, f in enumerate(fib)])
    rng.shuffle(lits)
    out.append(lits.tobytes())
    out.append(r(LIMIT - 1, 16))                                # the longest body taken on the device
    out.append(r(LIMIT - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- tests
def test_fixture_payloads_come_back_exactly(deflate):
    """independent of the runtime zlib: the reference's own deflated bytes"""
    pays = _fixture_payloads()
    assert len(pays) > 20
    bodies = [zlib.decompress(p, wbits=-15) for p in pays]
    res, outside, _, _ = deflate(bodies)
    bad = [i for i, (p, (st, got)) in enumerate(zip(pays, res)) if st != 0 or got != p]
    assert not bad, f"{len(bad)} of {len(pays)} fixture payloads differ (first: {bad[:5]})"
    if outside is not None:
        assert (outside == 0xAB).all()


def test_fixture_bodies_match_zlib(deflate):
    bodies = _fixture_bodies()
    res, outside, _, _ = deflate(bodies)
    for i, (b, (st, got)) in enumerate(zip(bodies, res)):
        assert st == 0 and got == _zlib(b), f"body {i} ({len(b)} bytes)"
        assert zlib.decompress(got, wbits=-15) == b
    if outside is not None:
        assert (outside == 0xAB).all()


def test_edge_bodies_match_zlib(deflate):
    bodies = _edge_bodies()
    res, outside, _, _ = deflate(bodies)
    types = set()
    for i, (b, (st, got)) in enumerate(zip(bodies, res)):
        ref = _zlib(b)
        assert st == 0 and got == ref, f"body {i} ({len(b)} bytes): {len(got)} vs zlib's {len(ref)} bytes"
        assert zlib.decompress(got, wbits=-15) == b
        types.add(got[0] >> 1 & 3)
    assert types == {0, 1, 2}                                  # stored, fixed and dynamic blocks all occur
    assert res[0][1] == b"\x03\x00"
    if outside is not None:
        assert (outside == 0xAB).all()


def test_each_body_alone_in_its_own_launch(deflate):
    """a launch's LDS follows its stride: the small bodies again, each in a launch sized for itself"""
    for b in _edge_bodies()[:12]:
        res, outside, _, _ = deflate([b])
        assert res[0] == (0, _zlib(b))
        if outside is not None:
            assert (outside == 0xAB).all()


def test_large_bodies_are_left_to_the_host(deflate):
    rng = np.random.default_rng(9)
    bodies = [rng.integers(0, 8, LIMIT, dtype=np.uint8).tobytes(), b"abc" * 1000, bytes(70000),
              rng.integers(0, 8, LIMIT - 1, dtype=np.uint8).tobytes()]
    res, outside, rows, nb = deflate(bodies)
    assert [r[0] for r in res] == [1, 0, 1, 0]
    assert res[1][1] == _zlib(bodies[1]) and res[3][1] == _zlib(bodies[3])
    assert nb[0] == 0 and nb[2] == 0
    if outside is not None:                                    # the emulator's rows start as 0xAB: untouched
        assert (rows[0] == 0xAB).all() and (rows[2] == 0xAB).all()
        assert (outside == 0xAB).all()


def test_row_too_small_is_status_2():
    em = EmuDeflate()
    bodies = [bytes(range(256)) * 4, b"abc"]
    res, outside, rows, _ = em(bodies, stride=160)
    assert res[0][0] == 2 and res[1] == (0, _zlib(b"abc"))
    assert (rows[0] == 0xAB).all() and (outside == 0xAB).all()


def test_stride_bound():
    from frad_python_amd._lib import FradLib
    lib = FradLib(build_emulator())
    assert lib.deflate_stride(0) == 16
    for n in (1, 100, 16382, 16383, 40000, LIMIT - 1):
        s = lib.deflate_stride(n)
        assert s % 16 == 0 and s >= n + 6 * (n // 16383 + 1) + 1
    assert lib.deflate_stride(10 ** 6) == lib.deflate_stride(LIMIT - 1)
    rng = np.random.default_rng(4)
    for n in (0, 1, 1000, 16383, 50000, LIMIT - 1):           # zlib's own worst case stays inside the bound
        assert len(_zlib(rng.integers(0, 256, n, dtype=np.uint8).tobytes())) <= n + 6 * (n // 16383 + 1) + 1


def test_abi_argument_checks():
    from frad_python_amd._lib import FradLib, FradError
    lib = FradLib(build_emulator())
    src = np.zeros(64, np.uint8)
    off = np.array([0, 10], np.int64)
    dst = np.zeros(256 + 16, np.uint8)
    base = dst.ctypes.data + (-dst.ctypes.data) % 16
    nb, st = np.zeros(1, np.int64), np.zeros(1, np.int32)
    for args in [(0, off.ctypes.data, 1, base, 64), (src.ctypes.data, 0, 1, base, 64), (src.ctypes.data, off.ctypes.data, 1, 0, 64),
                 (src.ctypes.data, off.ctypes.data, 1, base, 40), (src.ctypes.data, off.ctypes.data, 1, base + 1, 64),
                 (src.ctypes.data, off.ctypes.data, -1, base, 64)]:
        with pytest.raises(FradError):
            lib.deflate_raw(*args, nb.ctypes.data, st.ctypes.data)
    with pytest.raises(FradError):
        lib.deflate_raw(src.ctypes.data, off.ctypes.data, 1, base, 64, 0, st.ctypes.data)
    lib.deflate_raw(src.ctypes.data, off.ctypes.data, 0, base, 64, nb.ctypes.data, st.ctypes.data)   # nothing to do
    with pytest.raises(FradError):
        lib.deflate_stride(-1)


def test_deflate_batch_checks_its_arguments():
    import torch
    from frad_python_amd import core
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            core.deflate_batch(torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 4]))
        return
    src = torch.zeros(10, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 4, 10], dtype=torch.int64, device="cuda")
    core.deflate_batch(src, off)
    rows, nbytes, status = core.deflate_batch(src[:0], off[:1])          # an empty batch: empty results, nothing launched
    assert tuple(rows.shape) == (0, 16) and nbytes.dtype == torch.int64 and status.dtype == torch.int32
    assert nbytes.numel() == 0 and status.numel() == 0
    for bad in (torch.tensor([0, 11], device="cuda"), torch.tensor([0, 6, 4], device="cuda"), torch.tensor([-1, 4], device="cuda")):
        with pytest.raises(ValueError):
            core.deflate_batch(src, bad)
    with pytest.raises(ValueError):
        core.deflate_batch(src.to(torch.int32), off)
    with pytest.raises(ValueError):
        core.deflate_batch(src, off.to(torch.int32))
    with pytest.raises(ValueError):
        core.deflate_batch(src.view(2, 5), off)
    with pytest.raises(ValueError):
        core.deflate_batch(src, torch.zeros(0, dtype=torch.int64, device="cuda"))


# -------------------------------------------------------------------------------------------------------------- streams
def _pcm(n, C, seed=11):
    from frad_python_amd import synth
    return synth.to_pcm(synth.harmonic_mix(n, C, 48000, seed=seed), "s16le").tobytes()


def _encode(profile, pcm, C, fsize, overlap, pieces=(), loss=None, ecc_plan=None, **kw):
    """the stream of one Encoder fed `pcm` in the given pieces; ecc_plan: per call, None (leave) or a set_ecc argument"""
    from frad_python_amd.encoder import Encoder
    enc = Encoder(profile, 48000, C, 16, fsize, "s16le", allow_profile2=profile == 2, allow_ecc=ecc_plan is not None, **kw)
    enc.set_overlap_ratio(overlap)
    if loss is not None:
        enc.set_loss_level(loss)
    out, prev = [], 0
    cuts = [c for c in pieces if 0 < c < len(pcm)] + [len(pcm)]
    for k, c in enumerate(cuts):
        if ecc_plan is not None and ecc_plan[k % len(ecc_plan)] is not None:
            on, r = ecc_plan[k % len(ecc_plan)]
            enc.set_ecc(on, r)
        out.append(enc.process(pcm[prev:c]).buf)
        prev = c
    out.append(enc.flush().buf)
    return b"".join(out), enc


def _decode(stream: bytes, **kw) -> np.ndarray:
    from frad_python_amd.decoder import Decoder
    dec = Decoder(**kw)
    outs = [o for o in (dec.process(stream).pcm, dec.flush().pcm) if o.size]
    return np.concatenate(outs) if outs else np.array([])


def _same_streams(profile, pcm, C, fsize, overlap, **kw):
    ref, _ = _encode(profile, pcm, C, fsize, overlap, **kw)
    got, enc = _encode(profile, pcm, C, fsize, overlap, device_deflate=True, **kw)
    assert got == ref
    return got, enc


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 2])
@pytest.mark.parametrize("fsize,C", [(2048, 2), (512, 1), (1024, 3)])
@pytest.mark.parametrize("overlap", [0, 2, 16])
def test_device_deflate_streams_equal_the_default_path(profile, fsize, C, overlap):
    rng = np.random.default_rng(fsize * 7 + C + overlap)
    pcm = _pcm(fsize * 6 + 123, C, seed=fsize + C)
    step = 2 * C
    for loss in (None, 0.125, 4.0, 20.0):
        cuts = sorted(int(x) * step for x in rng.integers(1, len(pcm) // step, 3))
        _same_streams(profile, pcm, C, fsize, overlap, pieces=cuts, loss=loss)


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 2])
def test_device_deflate_with_ecc_toggled(profile):
    pcm = _pcm(2048 * 8 + 5, 2, seed=7)
    cuts = [2048 * 4 * k + 100 * k for k in range(1, 7)]
    plan = [(True, (96, 24)), None, (False, (96, 24)), (True, (200, 40)), (True, (0, 3)), (False, (10, 5))]
    s, _ = _same_streams(profile, pcm, 2, 2048, 16, pieces=cuts, ecc_plan=plan)
    a, b = _decode(s), _decode(s, device_inflate=True)
    assert a.size and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_device_deflate_large_frames_take_the_host_route():
    """N = 28 672 with 4 channels at a low loss level: bodies past 65 273 bytes are deflated by zlib, the rest on the device"""
    pcm = _pcm(28672 * 2 + 999, 4, seed=13)
    for profile in (1, 2):
        got, enc = _same_streams(profile, pcm, 4, 28672, 2, loss=0.125)
        assert enc.bridge.last_deflate_host >= 1
    import torch
    none = torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    assert enc.bridge.deflate_payloads(*none) == []                       # no bodies: no payloads, nothing launched


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [0, 4])
def test_device_deflate_ignored_by_lossless_profiles(profile):
    pcm = _pcm(2048 * 3 + 17, 2, seed=3)
    _same_streams(profile, pcm, 2, 2048, 0, pieces=(4000, 9000))


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 2])
def test_device_deflate_streams_decode(profile):
    pcm = _pcm(2048 * 5 + 321, 2, seed=21)
    s, _ = _same_streams(profile, pcm, 2, 2048, 16)
    a, b = _decode(s), _decode(s, device_inflate=True)
    assert a.size and a.tobytes() == b.tobytes()
