"""Raw DEFLATE inflate on the device (frad_inflate_raw, core.inflate_batch) and ``Decoder(device_inflate=True)``.

The kernel is checked against zlib on the CPU emulator (``emu``, the same kernel source) and on the MI355X (``gpu``): every
valid stream must give status 0 and zlib's bytes; for a damaged stream status 0 must mean that zlib accepts it with the same
bytes, and every stream zlib rejects must get a non-zero status.  End to end (GPU): the decoder's PCM with the device inflate
must be bit-identical to the host-inflate path's."""
import zlib

import numpy as np
import pytest

from helpers import build_emulator

GOLDEN = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden")
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def _zlib(x: bytes):
    try:
        return zlib.decompress(x, wbits=-15)
    except zlib.error:
        return None


def _deflate(data: bytes, level: int, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


# ------------------------------------------------------------------------------------------------------------- backends
class EmuInflate:
    def __init__(self):
        from frad_python_amd._lib import FradLib
        self.lib = FradLib(build_emulator())

    def __call__(self, streams, stride, guard=64):
        """-> [(status, bytes)], and the destination buffer's bytes outside the rows (must stay 0xAB)"""
        n = len(streams)
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in streams], out=off[1:])
        joined = b"".join(streams)                             # exactly the stream bytes: no slack to hide an over-read
        src = np.frombuffer(joined, np.uint8).copy() if joined else np.zeros(1, np.uint8)
        dst = np.full(n * stride + guard + 16, 0xAB, np.uint8)
        base = (-dst.ctypes.data) % 16
        nb = np.zeros(max(n, 1), np.int64)
        st = np.zeros(max(n, 1), np.int32)
        self.lib.inflate_raw(src.ctypes.data, off.ctypes.data, n, dst.ctypes.data + base, stride, nb.ctypes.data, st.ctypes.data)
        rows = dst[base:base + n * stride]
        out = [(int(st[i]), rows[i * stride:i * stride + nb[i]].tobytes()) for i in range(n)]
        return out, np.concatenate([dst[:base], dst[base + n * stride:]]), rows


class GpuInflate:
    def __init__(self):
        import torch
        from frad_python_amd import core
        self.torch, self.core = torch, core

    def __call__(self, streams, stride, guard=64):
        t = self.torch
        off = np.zeros(len(streams) + 1, np.int64)
        np.cumsum([len(s) for s in streams], out=off[1:])
        src = t.from_numpy(np.frombuffer(b"".join(streams) + b"\0", np.uint8).copy()).cuda()[:int(off[-1])]
        dst, nb, st = self.core.inflate_batch(src, t.from_numpy(off).cuda(), stride)
        rows, nb, st = dst.cpu().numpy().reshape(-1), nb.cpu().numpy(), st.cpu().numpy()
        return [(int(st[i]), rows[i * stride:i * stride + nb[i]].tobytes()) for i in range(len(streams))], None, rows


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def inflate(request):
    return EmuInflate() if request.param == "emu" else GpuInflate()


# --------------------------------------------------------------------------------------------------------------- corpus
def _oracle_bodies():
    """inflated profile-1 bodies (the oracle's deflated frames, g4) and profile-2 bodies (the oracle's pre-deflate bodies, g8)"""
    g4 = np.load(f"{GOLDEN}/g4_p1.npz")
    p1 = [zlib.decompress(g4[k].tobytes(), wbits=-15) for k in g4.files if k.endswith("_frad")]
    g8 = np.load(f"{GOLDEN}/g8_p2_enc.npz")
    off = g8["body_off"]
    p2 = [g8["body"][off[i]:off[i + 1]].tobytes() for i in range(0, len(off) - 1, 7)]
    return p1, p2


def _valid_corpus():
    p1, p2 = _oracle_bodies()
    out = []
    for body in p1[:3] + p2[:3]:
        for level in range(10):
            for s in STRATEGIES:
                out.append((body, _deflate(body, level, s)))
    rng = np.random.default_rng(7)
    for n in (1, 100, 5000):                                    # random bytes: stored blocks
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out.append((d, _deflate(d, 6)))
    for level in (0, 1, 6, 9):                                 # empty bodies
        out.append((b"", _deflate(b"", level)))
    return out


def test_valid_streams_match_zlib(inflate):
    corpus = _valid_corpus()
    assert len(corpus) > 300 and len({s for _, s in corpus}) > 60      # (bodies of Golomb codes: many settings agree)
    res, outside, _ = inflate([s for _, s in corpus], 18176)
    bad = [i for i, ((d, _), (st, got)) in enumerate(zip(corpus, res)) if st != 0 or got != d]
    assert not bad, f"{len(bad)} of {len(corpus)} valid streams differ from zlib (first: {bad[:5]})"
    if outside is not None:
        assert (outside == 0xAB).all()


def test_long_streams_ring_window(inflate):
    """outputs beyond 32 KiB (the ring window), several blocks, distances near 32 768"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 33000, dtype=np.uint8).tobytes()
    far = a[:32768] + a[:2000] + rng.integers(0, 4, 20000, dtype=np.uint8).tobytes() + a[40:32000]
    datas = [far, rng.integers(0, 256, 150000, dtype=np.uint8).tobytes(), b"frad " * 30000]
    streams = [(d, _deflate(d, lv)) for d in datas for lv in (0, 1, 9)]
    for stride in (160000, 262144):
        res, outside, _ = inflate([s for _, s in streams], stride)
        for (d, s), (st, got) in zip(streams, res):
            if len(d) <= stride:
                assert st == 0 and got == d
            else:
                assert st == 2
        if outside is not None:
            assert (outside == 0xAB).all()
    # the copy of a[:2000] lies 32 768 bytes back
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9)
    s = c.compress(far) + c.flush()
    res, _, _ = inflate([s], 98304)
    assert res[0] == (0, far)


def test_output_overflow_is_status_2_and_stays_in_the_row(inflate):
    d = bytes(range(256)) * 8
    streams = [_deflate(d, 6), _deflate(d, 0), _deflate(b"x" * 100, 9)]
    res, outside, rows = inflate(streams, 1024)
    assert [r[0] for r in res] == [2, 2, 0]
    assert res[2][1] == b"x" * 100
    if outside is not None:                                     # the emulator's buffer has guard bytes on both sides
        assert (outside == 0xAB).all()
        assert (rows[2 * 1024 + 100:] == 0xAB).all()        # only the bytes of the output are written


# ------------------------------------------------------------------------------------------------------ hand-built streams
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        return self

    def code(self, code, length):                             # Huffman codes go MSB first
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """RFC 1951 3.2.2 code assignment (for any lengths: a broken code gets codes all the same)"""
    bl = [0] * 17
    for ln in lengths:
        bl[ln] += 1
    bl[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_OK = [4] * 13 + [5] * 6                                      # a complete code-length code over all 19 symbols


def dynamic(b, lit, dist, data, final=1, clen=CL_OK, cl_syms=None):
    """one dynamic block.  data: ints (literal / length symbols without extra bits), ("m", lsym, lextra, nlbits, dsym,
    dextra, ndbits) for a match, ("d", dsym) for a bare distance code, ("bits", value, n) for raw bits"""
    b.put(final, 1).put(2, 2).put(len(lit) - 257, 5).put(len(dist) - 1, 5).put(15, 4)
    for i in range(19):
        b.put(clen[ORDER[i]], 3)
    cc = canonical(clen)
    for s in (cl_syms if cl_syms is not None else [(ln, 0, 0) for ln in list(lit) + list(dist)]):
        sym, extra, nb = s
        b.code(*cc[sym]).put(extra, nb)
    lc, dc = canonical(lit), canonical(dist)
    for x in data:
        if isinstance(x, int):
            b.code(*lc[x])
        elif x[0] == "m":
            _, ls, le, nl, ds, de, nd = x
            b.code(*lc[ls]).put(le, nl).code(*dc[ds]).put(de, nd)
        elif x[0] == "bits":
            b.put(x[1], x[2])
        else:
            b.code(*dc[x[1]])
    return b


def _lit(pairs, n=286):
    v = [0] * n
    for s, ln in pairs.items():
        v[s] = ln
    return v


LIT = _lit({97: 2, 98: 2, 256: 2, 257: 2})                     # complete: 4 codes of 2 bits
DIST = [1, 1] + [0] * 28                                        # complete: 2 codes of 1 bit
GOOD = [97, 98, ("m", 257, 0, 0, 0, 0, 0), 256]                 # "ab" + copy 3 from distance 1 -> "abbbb"


def fixed(b, syms, final=1):
    """a fixed-code block; syms: literal/length symbols, or ("d", dsym) for a 5-bit distance code"""
    b.put(final, 1).put(1, 2)
    for s in syms:
        if isinstance(s, tuple):
            b.code(s[1], 5)
        elif s < 144:
            b.code(0x30 + s, 8)
        elif s < 256:
            b.code(0x190 + s - 144, 9)
        elif s < 280:
            b.code(s - 256, 7)
        else:
            b.code(0xC0 + s - 280, 8)
    return b


def hand_built():
    """(name, stream, zlib accepts?)"""
    z = [(16, 0, 2)]
    cases = [
        ("good dynamic", dynamic(Bits(), LIT, DIST, GOOD).bytes(), True),
        ("empty input", b"", False),
        ("btype 3", Bits().put(1, 1).put(3, 2).bytes(), False),
        ("stored len/nlen mismatch", Bits().put(1, 1).put(0, 2).align().put(5, 16).put(0, 16).bytes() + b"hello", False),
        ("stored, length 0", Bits().put(1, 1).put(0, 2).align().put(0, 16).put(0xFFFF, 16).bytes(), True),
        ("stored 0 + fixed + final stored", fixed(Bits().put(0, 1).put(0, 2).align().put(0, 16).put(0xFFFF, 16), [104, 105, 256],
                                                  final=0).put(1, 1).put(0, 2).align().put(3, 16).put(0xFFFC, 16).bytes() + b"xyz", True),
        ("stored 0 + fixed + stored, no final block", fixed(Bits().put(0, 1).put(0, 2).align().put(0, 16).put(0xFFFF, 16),
                                                            [104, 105, 256], final=0).put(0, 1).put(0, 2).align().put(3, 16)
         .put(0xFFFC, 16).bytes() + b"xyz", False),
        ("hlit 287", dynamic(Bits(), LIT + [0], DIST, GOOD).bytes(), False),
        ("hdist 31", dynamic(Bits(), LIT, DIST + [0], GOOD).bytes(), False),
        ("repeat 16 first", dynamic(Bits(), LIT, DIST, GOOD, cl_syms=z + [(0, 0, 0)] * 313).bytes(), False),
        ("repeat past hlit+hdist", dynamic(Bits(), LIT, DIST, GOOD,
                                           cl_syms=[(18, 127, 7), (18, 127, 7), (18, 127, 7)]).bytes(), False),
        ("over-subscribed literal code", dynamic(Bits(), _lit({97: 1, 98: 2, 256: 2, 257: 2}), DIST, GOOD).bytes(), False),
        ("incomplete literal code", dynamic(Bits(), _lit({97: 2, 256: 2, 257: 2}), DIST, [97, 256]).bytes(), False),
        ("single 1-bit literal code (EOB)", dynamic(Bits(), _lit({256: 1}), [0] * 30, [256]).bytes(), True),
        ("no end-of-block code", dynamic(Bits(), _lit({97: 1, 98: 1}), DIST, [97]).bytes(), False),
        ("empty distance code, literals only", dynamic(Bits(), _lit({97: 1, 256: 1}), [0] * 30, [97, 97, 256]).bytes(), True),
        ("empty distance code, a match", dynamic(Bits(), LIT, [0] * 30, [97, 257, ("bits", 0, 8), 256]).bytes(), False),
        ("single 1-bit distance code", dynamic(Bits(), LIT, [1] + [0] * 29, GOOD).bytes(), True),
        ("single 1-bit distance code, unused code", dynamic(Bits(), LIT, [1] + [0] * 29, [97, 257]).put(1, 1).put(0, 8).bytes(), False),
        ("incomplete distance code (2 bits)", dynamic(Bits(), LIT, [2] + [0] * 29, GOOD).bytes(), False),
        ("incomplete code-length code", dynamic(Bits(), LIT, DIST, GOOD, clen=[0, 2, 2] + [0] * 16,
                                                 cl_syms=[(1, 0, 0)] * 10).bytes(), False),
        ("over-subscribed code-length code", dynamic(Bits(), LIT, DIST, GOOD, clen=[1, 1, 1] + [0] * 16,
                                                     cl_syms=[(1, 0, 0)] * 10).bytes(), False),
        ("single 1-bit code-length code", dynamic(Bits(), LIT, DIST, GOOD, clen=[1] + [0] * 18, cl_syms=[(0, 0, 0)] * 10).bytes(), False),
        ("fixed literal/length 286", fixed(Bits(), [97, 286, 256]).bytes(), False),
        ("fixed literal/length 287", fixed(Bits(), [97, 287, 256]).bytes(), False),
        ("fixed distance 30", fixed(Bits(), [97, 257, ("d", 30), 256]).bytes(), False),
        ("fixed distance 31", fixed(Bits(), [97, 257, ("d", 31), 256]).bytes(), False),
        ("distance too far back", fixed(Bits(), [97, 257, ("d", 1), 256]).bytes(), False),
        ("distance = bytes so far", fixed(Bits(), [97, 98, 257, ("d", 1), 256]).bytes(), True),
        ("fixed, no end-of-block", fixed(Bits(), [97, 98]).bytes(), False),
        ("trailing bytes after the final block", dynamic(Bits(), LIT, DIST, GOOD).bytes() + b"\x07garbage", True),
        ("non-final block, input ends", fixed(Bits(), [97, 256], final=0).bytes(), False),
        ("two blocks", fixed(fixed(Bits(), [97, 256], final=0), [98, 257, ("d", 0), 256]).bytes(), True),
    ]
    return cases


def test_hand_built_streams_follow_zlib(inflate):
    cases = hand_built()
    for name, s, ok in cases:                                   # the corpus says what it claims
        assert (_zlib(s) is not None) == ok, name
    res, _, _ = inflate([s for _, s, _ in cases], 1024)
    for (name, s, ok), (st, got) in zip(cases, res):
        ref = _zlib(s)
        if ok:
            assert st == 0 and got == ref, name
        else:
            assert st == 1, name


def _damaged_corpus():
    p1, p2 = _oracle_bodies()
    small = _deflate(b"the quick brown fox jumps over the lazy dog " * 12 + bytes(range(256)), 9)
    streams = [_deflate(p1[0], 6), _deflate(p2[0], 9, zlib.Z_FIXED), small]
    out = []
    for s in streams[1:]:                                        # truncations at every length
        out += [s[:k] for k in range(len(s))]
    for j, s in enumerate(streams):                              # single-bit flips
        step = 1 if j == 2 else 5
        for k in range(j, len(s) * 8, step):
            b = bytearray(s)
            b[k // 8] ^= 1 << (k % 8)
            out.append(bytes(b))
    return out


def test_damaged_streams_never_differ_from_zlib(inflate):
    corpus = _damaged_corpus()
    stride = 18304
    res, outside, _ = inflate(corpus, stride)
    wrong = over_strict = rejected = 0
    for s, (st, got) in zip(corpus, res):
        ref = _zlib(s)
        if st == 0 and got != ref:
            wrong += 1
        if ref is None:
            rejected += 1
            assert st != 0
        elif st != 0 and len(ref) <= stride:
            over_strict += 1
    print(f"damaged streams: {len(corpus)}, zlib rejects {rejected}, device rejects where zlib accepts: {over_strict}")
    assert wrong == 0
    assert over_strict == 0
    assert 100 < rejected < len(corpus)
    if outside is not None:
        assert (outside == 0xAB).all()


def test_abi_argument_checks():
    from frad_python_amd._lib import FradError, FradLib
    lib = FradLib(build_emulator())
    src = np.zeros(64, np.uint8)
    off = np.array([0, 1], np.int64)
    dst = np.zeros(256, np.uint8)
    p = dst.ctypes.data + (-dst.ctypes.data) % 16
    nb, st = np.zeros(1, np.int64), np.zeros(1, np.int32)
    for stride, d in ((24, p), (0, p), (32, p + 1)):
        with pytest.raises(FradError):
            lib.inflate_raw(src.ctypes.data, off.ctypes.data, 1, d, stride, nb.ctypes.data, st.ctypes.data)
    with pytest.raises(FradError):
        lib.inflate_raw(src.ctypes.data, off.ctypes.data, -1, p, 32, nb.ctypes.data, st.ctypes.data)
    lib.inflate_raw(0, 0, 0, 0, 32, 0, 0)                      # an empty batch is a no-op


@pytest.mark.gpu
def test_inflate_batch_checks_its_arguments():
    import torch
    from frad_python_amd import core
    src = torch.zeros(10, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 4, 10], dtype=torch.int64, device="cuda")
    core.inflate_batch(src, off, 32)
    rows, nbytes, status = core.inflate_batch(src[:0], off[:1], 32)      # an empty batch: empty results, nothing launched
    assert tuple(rows.shape) == (0, 32) and nbytes.dtype == torch.int64 and status.dtype == torch.int32
    assert nbytes.numel() == 0 and status.numel() == 0
    with pytest.raises(ValueError):
        core.inflate_batch(src, off, 24)
    with pytest.raises(ValueError):
        core.inflate_batch(src, torch.tensor([0, 11], dtype=torch.int64, device="cuda"), 32)
    with pytest.raises(ValueError):
        core.inflate_batch(src, torch.tensor([0, 5, 4], dtype=torch.int64, device="cuda"), 32)
    with pytest.raises(ValueError):
        core.inflate_batch(src, off.to(torch.int32), 32)
    with pytest.raises(ValueError):
        core.inflate_batch(src.view(2, 5), off, 32)


# -------------------------------------------------------------------------------------------------------------- streams
def _decode(stream: bytes, pieces=None, **kw):
    from frad_python_amd.decoder import Decoder
    dec = Decoder(**kw)
    outs = []
    if pieces is None:
        outs.append(dec.process(stream).pcm)
    else:
        prev = 0
        for c in list(pieces) + [len(stream)]:
            outs.append(dec.process(stream[prev:c]).pcm)
            prev = c
    outs.append(dec.flush().pcm)
    outs = [o for o in outs if o.size]
    return np.concatenate(outs) if outs else np.array([])


def _same(stream, pieces=None, **kw):
    ref = _decode(stream, pieces, **kw)
    got = _decode(stream, pieces, device_inflate=True, **kw)
    assert ref.dtype == got.dtype and ref.shape == got.shape
    assert ref.tobytes() == got.tobytes()
    return ref


def _encode(profile, pcm, C, fsize, overlap, bits=16, ecc=None, loss=None):
    from frad_python_amd.encoder import Encoder
    enc = Encoder(profile, 48000, C, bits, fsize, "s16le", allow_profile2=profile == 2, allow_ecc=ecc is not None)
    enc.set_overlap_ratio(overlap)
    if loss is not None:
        enc.set_loss_level(loss)
    if ecc is not None:
        enc.set_ecc(True, ecc)
    return enc.process(pcm).buf + enc.flush().buf


def _pcm(n, C, seed=11):
    from frad_python_amd import synth
    return synth.to_pcm(synth.harmonic_mix(n, C, 48000, seed=seed), "s16le").tobytes()


def _payload_offsets(s) -> list:
    from frad_python_amd.tools.asfh import ASFH
    pos, out = 0, []
    while pos < len(s):
        a = ASFH()
        a.read(bytes(s[pos:pos + 40]))
        pos += a.header_bytes
        out.append(pos)
        pos += a.frmbytes
    return out


@pytest.mark.gpu
def test_device_inflate_golden_streams():
    g3 = np.load(f"{GOLDEN}/g3_p1_streams.npz")
    for k in g3.files:
        if k.endswith("_stream"):
            _same(g3[k].tobytes())
            _same(g3[k].tobytes(), out_format="s16le")
    g7 = np.load(f"{GOLDEN}/g7_p2.npz")
    off = g7["stream_off"]
    for i in range(len(off) - 1):
        _same(g7["stream"][off[i]:off[i + 1]].tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [1, 2])
@pytest.mark.parametrize("fsize,C", [(2048, 2), (512, 1), (1024, 3)])
@pytest.mark.parametrize("overlap", [0, 2, 16])
def test_device_inflate_encoder_streams(profile, fsize, C, overlap):
    pcm = _pcm(fsize * 5 + 77, C, seed=fsize + C)
    s = _encode(profile, pcm, C, fsize, overlap)
    for fmt in (None, "s16le"):
        ref = _same(s, out_format=fmt)
        assert ref.size
    _same(s, pieces=(1, 333, len(s) // 2, len(s) - 5))


@pytest.mark.gpu
def test_device_inflate_large_frames_ring_window():
    """a frame whose bound exceeds 32 KiB (the ring-window kernel) and a loss level that keeps every coefficient"""
    pcm = _pcm(4096 * 3, 8, seed=5)
    for profile in (1, 2):
        _same(_encode(profile, pcm, 8, 4096, 2, loss=0.0))


@pytest.mark.gpu
def test_device_inflate_ecc_streams_with_repair():
    pcm = _pcm(2048 * 6, 2, seed=3)
    for profile in (1, 2):
        s = bytearray(_encode(profile, pcm, 2, 2048, 16, ecc=(96, 24)))
        for k, p in enumerate(_payload_offsets(s)[1:4]):
            s[p + 5 + k] ^= 0x5A                                 # one byte error in the first block of three payloads
        _same(bytes(s), fix_error=True)


@pytest.mark.gpu
def test_device_inflate_run_fallback_keeps_the_zero_frame():
    """a payload zlib rejects: the run goes through the host-inflate path and the frame decodes as zeros, as before"""
    pcm = _pcm(2048 * 6, 2, seed=9)
    for profile in (1, 2):
        for overlap in (0, 16):
            s = bytearray(_encode(profile, pcm, 2, 2048, overlap))
            p = _payload_offsets(s)[2]
            s[p] = 0x07                                          # BFINAL = 1, BTYPE = 3: no DEFLATE stream
            assert _zlib(bytes(s[p:p + 64])) is None
            ref = _same(bytes(s))
            assert ref.size


@pytest.mark.gpu
def test_device_inflate_run_costs_the_same_calls_whatever_its_length(monkeypatch):
    """device_inflate=True: the fused run from the deflated payloads on makes the same C-ABI calls for 8 frames and for 64"""
    from test_stream import decoder_call_counts
    few, many = decoder_call_counts(monkeypatch, 1, 2048, 2, 16, 16, device_inflate=True)
    assert few == many and few["inflate_raw"] == 1
