"""Profile 2 (TNS) decoding (fourier/profile2.py:58-91, tools/p2tools.py) against the reference's own outputs (g7_p2.npz, written
by tools/gen_golden_p2.py) and a host model.  "emu": the CPU interpreter of the same kernel source (frad_golomb.hip, frad_p1.hip,
the inverse DCT, the cross-fade); "gpu": the MI355X through HipBridge."""
import zlib

import numpy as np
import pytest
from scipy import signal as ss

from conftest import load_npz
from frad_python_amd import Decoder, Encoder, Repairer
from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64, pcm_dtype_code
from oracle import frad_oracle as fo

P2_DEPTHS = (8, 10, 12, 14, 16, 20, 24)


# --------------------------------------------------------------------------------------------------------- backends
class EmuP2Bridge:
    """The decoder's bridge interface for profile 2 on the CPU interpreter build, with numpy buffers."""

    def __init__(self):
        from test_ecc import EmuEcc
        self.rs = EmuEcc()
        self.lib = self.scan_lib = self.rs.lib
        self.rs_encode, self.rs_repair = self.rs.rs_encode, self.rs.rs_repair

    def ints(self, bodies, N, C):
        off = np.zeros(len(bodies) + 1, np.int64)
        np.cumsum([len(b) for b in bodies], out=off[1:])
        flat = np.frombuffer(b"".join(bodies) + bytes(16), np.uint8).copy()
        n = len(bodies)
        q = np.full((max(n, 1), N, C), -7, np.int32); tq = np.full((max(n, 1), 27, C), -7, np.int32)
        lpc = np.full((max(n, 1), 13, C), -7, np.int32); st = np.full(max(n, 1), -7, np.int32)
        self.lib.p2_golomb_decode(flat.ctypes.data, off.ctypes.data, n, N, C, q.ctypes.data, tq.ctypes.data, lpc.ctypes.data, st.ctypes.data)
        return q[:n], tq[:n], lpc[:n], st[:n]

    def synth(self, q, tq, lpc, N, C, bits, srate):
        n = q.shape[0]
        q, tq, lpc = (np.ascontiguousarray(a, np.int32) for a in (q, tq, lpc))
        out = np.zeros((max(n, 1), N, C))
        self.lib.p2_synth(q.ctypes.data, tq.ctypes.data, lpc.ctypes.data, n, N, C, bits, srate, out.ctypes.data)
        return out[:n]

    def digital(self, q, tq, lpc, N, C, bits, srate):
        coeffs = self.synth(q, tq, lpc, N, C, bits, srate)
        n = coeffs.shape[0]
        out = np.zeros((max(n, 1), N, C))
        self.lib.p0_digital(coeffs.ctypes.data, N * C * 8, n, N, C, 64, 1, out.ctypes.data)
        return out[:n]

    def p1_digital(self, q, tq, N, C, bits, srate):
        n = q.shape[0]
        q, tq = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(tq, np.int32)
        out = np.zeros((max(n, 1), N, C))
        self.lib.p1_digital(q.ctypes.data, tq.ctypes.data, n, N, C, bits, srate, out.ctypes.data)
        return out[:n]

    def p2_decode_bodies(self, bodies, N, C, bits, srate):
        q, tq, lpc, _ = self.ints(bodies, N, C)
        return self.digital(q, tq, lpc, N, C, bits, srate)

    def p2_decode_run(self, bodies, N, C, bits, srate, ratio, prev_tail, out_format=None):
        frames = np.ascontiguousarray(self.p2_decode_bodies(bodies, N, C, bits, srate))
        n = frames.shape[0]
        cut = N * (ratio - 1) // ratio
        pt = np.ascontiguousarray(prev_tail, np.float64) if prev_tail is not None else None
        nxt = np.zeros((N - cut, C))
        if out_format is not None and out_format != "f64le":
            dt = ff_format_to_numpy_type(out_format)
            out = np.zeros(n * cut * C * dt.itemsize + 16, np.uint8)
            self.lib.p1_overlap_add_pcm(frames.ctypes.data, n, N, C, ratio, pt.ctypes.data if pt is not None else 0,
                                        pcm_dtype_code(out_format), out.ctypes.data, nxt.ctypes.data)
            return np.frombuffer(out[:n * cut * C * dt.itemsize].tobytes(), dt).reshape(-1, C), nxt
        out = np.zeros((max(n, 1), cut, C))
        self.lib.p1_overlap_add(frames.ctypes.data, n, N, C, ratio, pt.ctypes.data if pt is not None else 0, out.ctypes.data, nxt.ctypes.data)
        return out[:n].reshape(-1, C), nxt


class GpuP2:
    """The same interface on the MI355X: core's batched wrappers, the decoder through HipBridge."""

    def __init__(self):
        import torch
        from frad_python_amd import core
        from frad_python_amd.bridge import HipBridge
        self.t, self.core, self.bridge = torch, core, HipBridge()
        self.dev = self.bridge.device

    def _d(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.dev)

    def ints(self, bodies, N, C):
        return tuple(x.cpu().numpy() for x in self.bridge._p2_integers(bodies, N, C))

    def synth(self, q, tq, lpc, N, C, bits, srate):
        return self.core.p2_synth_batch(self._d(q), self._d(tq), self._d(lpc), N, C, bits, srate).cpu().numpy()

    def digital(self, q, tq, lpc, N, C, bits, srate):
        return self.core.p2_digital_batch(self._d(q), self._d(tq), self._d(lpc), N, C, bits, srate).cpu().numpy()

    def p1_digital(self, q, tq, N, C, bits, srate):
        return self.core.p1_digital_batch(self._d(q), self._d(tq), N, C, bits, srate).cpu().numpy()


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


@pytest.fixture(scope="module")
def be(kind):
    return EmuP2Bridge() if kind == "emu" else GpuP2()


def bridge_of(be):
    return be if isinstance(be, EmuP2Bridge) else be.bridge


@pytest.fixture(scope="module")
def g7():
    return load_npz("g7_p2.npz")


def frames_of(g7):
    """(index, N, C, depth index, rate, payload, reference PCM rows, row step): frames above 2048 store every 8th row"""
    d = g7
    for i, (N, C, fb, sr, step) in enumerate(d["meta"].tolist()):
        pay = d["payload"][d["payload_off"][i]:d["payload_off"][i + 1]].tobytes()
        pcm = d["pcm"][d["pcm_off"][i]:d["pcm_off"][i + 1]].reshape(-1, C)
        assert len(pcm) == (N + step - 1) // step
        yield i, N, C, fb, sr, pay, pcm, step


def streams_of(g7):
    d = g7
    for i, (ratio, bits, fsize, srate, C, rows) in enumerate(d["stream_meta"].tolist()):
        s = d["stream"][d["stream_off"][i]:d["stream_off"][i + 1]].tobytes()
        pcm = d["stream_pcm"][d["stream_pcm_off"][i]:d["stream_pcm_off"][i + 1]].reshape(rows, C)
        yield ratio, s, pcm


def close(got, ref, rel=1e-9):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= rel * scale, f"max |got - ref| = {err:.3e} > {rel:g} * {scale:.3g}"
    return err / scale


# --------------------------------------------------------------------------------------------------------- host model
def model_body(lpc_flat, tq_flat, q_flat) -> bytes:
    """profile2.analogue's packing (profile2.py:48-51) of given integers"""
    lg, tg, fg = fo.golomb_encode(np.asarray(lpc_flat)), fo.golomb_encode(np.asarray(tq_flat)), fo.golomb_encode(np.asarray(q_flat))
    return len(lg).to_bytes(2, "big") + lg + len(tg).to_bytes(4, "big") + tg + fg


def model_coeffs(q, tq, lpc, N, C, bits, srate):
    """profile2.py:69-84 + p2tools.tns_synthesis from integer arrays [N, C], [27, C], [13, C] -> [N, C] (before the IDCT)"""
    f = fo.dequant(np.asarray(q, float)) / 2.0 ** (bits - 1)
    out = np.zeros((N, C))
    with np.errstate(all="ignore"):
        t = np.power(np.e / 2, fo.quant(np.asarray(tq, float)))
        for c in range(C):
            x = f[:, c]
            if np.any(lpc[:, c]):
                a = np.concatenate([[1.0], lpc[1:, c].astype(float) / 15])
                y = ss.lfilter([1], a, x)
                if not (np.any(np.isnan(y)) or np.any(np.isinf(y)) or np.max(np.abs(y)) > 1e6):
                    x = y
            out[:, c] = x * fo.spread_thresholds(t[:, c], N, srate)
    return out


def rand_ints(rng, N, C, lpc_rows=None):
    q = rng.integers(-40, 41, (N, C)).astype(np.int32)
    q[N // 2:] //= 8
    tq = rng.integers(0, 40, (27, C)).astype(np.int32)
    lpc = np.zeros((13, C), np.int32) if lpc_rows is None else np.asarray(lpc_rows, np.int32).reshape(13, C)
    return q, tq, lpc


# --------------------------------------------------------------------------------------------------------- whole streams
def decode(br, stream, cuts=(), **kw):
    dec = Decoder(bridge=br, **kw)
    pieces, last = [], 0
    for c in list(cuts) + [len(stream)]:
        pieces.append(dec.process(stream[last:c]).pcm)
        last = c
    pieces.append(dec.flush().pcm)
    C = 2
    return np.concatenate([p.reshape(-1, C) for p in pieces if p.size])


def test_streams_decode_like_the_reference(be, g7):
    """Today's failure: the decoder raised NotImplementedError on the first profile-2 header."""
    for ratio, s, ref in streams_of(g7):
        close(decode(bridge_of(be), s), ref)


def test_stream_overlap_tail_carries_across_calls(be, g7):
    rng = np.random.default_rng(7)
    for ratio, s, ref in streams_of(g7):
        whole = decode(bridge_of(be), s)
        for _ in range(2):
            cuts = sorted(rng.choice(np.arange(1, len(s)), 5, replace=False).tolist())
            got = decode(bridge_of(be), s, cuts)
            assert got.shape == whole.shape and np.array_equal(got, whole), f"ratio {ratio}: split at {cuts} changes the PCM"


@pytest.mark.parametrize("fmt", ["s16le", "f32le", "s32be"])
def test_stream_out_format_matches_host_conversion(be, g7, fmt):
    for ratio, s, ref in streams_of(g7):
        f64 = decode(bridge_of(be), s)
        got = decode(bridge_of(be), s, out_format=fmt)
        want = from_f64(f64, fmt)
        assert got.dtype.kind == want.dtype.kind and got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape
        assert np.array_equal(got, want), f"ratio {ratio} {fmt}"           # (values: the helper's concatenate drops a '>' order)


def test_repairer_protects_and_decoder_repairs_profile2(be, g7):
    rng = np.random.default_rng(11)
    br = bridge_of(be)
    for ratio, s, ref in streams_of(g7):
        clean = decode(br, s)
        r = Repairer((96, 24), bridge=br)
        prot = r.process(s) + r.process(b"") + r.flush()
        table, _, _ = br.scan_lib.asfh_scan(prot, 0)
        rows = table.tolist()
        assert rows and all(row[3] == 2 and row[4] for row in rows if not row[13])       # profile 2, ecc bit set
        dmg = bytearray(prot)
        for row in rows:
            p_off, p_len = row[1], row[2]
            for b0 in range(0, p_len, 120):                                              # <= 8 byte errors per 120-byte block
                blk = min(120, p_len - b0)
                for pos in rng.choice(blk, min(8, blk), replace=False):
                    dmg[p_off + b0 + int(pos)] ^= int(rng.integers(1, 256))
        close(decode(br, bytes(dmg), fix_error=True), clean, rel=0.0)


def test_stream_with_a_frame_that_does_not_inflate(be, g7):
    """profile2.py:63-64: a payload zlib rejects decodes to a frame of zeros, nothing raises"""
    br = bridge_of(be)
    ratio, s, ref = next(x for x in streams_of(g7) if x[0] == 0)
    table, _, _ = br.scan_lib.asfh_scan(s, 0)
    rows = [r for r in table.tolist() if not r[13]]
    k = 2
    p_off, p_len, fsize = rows[k][1], rows[k][2], rows[k][9]
    bad = bytearray(s)
    bad[p_off:p_off + p_len] = b"\xff" * p_len                                   # BTYPE = 3: not a deflate stream
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(bad[p_off:p_off + p_len]), wbits=-15)
    got, clean = decode(br, bytes(bad)), decode(br, s)
    want = clean.copy()
    want[k * fsize:(k + 1) * fsize] = 0.0
    assert np.array_equal(got, want)


def test_encoder_still_refuses_profile2():
    with pytest.raises(SystemExit):
        Encoder(2, 48000, 2, 16, 2048, "s16le")


# --------------------------------------------------------------------------------------------------------- per frame
def test_frames_match_the_reference(be, kind, g7):
    worst = 0.0
    for i, N, C, fb, sr, pay, ref, step in frames_of(g7):
        if kind == "emu" and N > 4096:
            continue                                         # the interpreter's inverse DCT at 28 672 takes minutes; the GPU run covers it
        got = bridge_of(be).p2_decode_bodies([zlib.decompress(pay, wbits=-15)], N, C, P2_DEPTHS[fb], sr)[0]
        worst = max(worst, close(got[::step], ref))
    print(f"\n[p2] worst per-frame |got - ref| / max(1, |ref|) on {kind}: {worst:.3e}")


def test_integers_match_the_host_decoder(be, g7):
    """frad_p2_golomb_decode == the three exp_golomb_rice_decode calls + untrim"""
    for i, N, C, fb, sr, pay, ref, step in frames_of(g7):
        if N > 4096:
            continue
        body = zlib.decompress(pay, wbits=-15)
        q, tq, lpc, st = be.ints([body], N, C)
        n = int.from_bytes(body[:2], "big")
        rest = body[2 + n:]
        t = int.from_bytes(rest[:4], "big")
        pad = lambda v, m: np.pad(v, (0, max(0, m - len(v))))[:m]     # noqa: E731
        assert st[0] == 0
        assert np.array_equal(lpc[0].reshape(-1), pad(fo.golomb_decode(body[2:2 + n]), 13 * C))
        assert np.array_equal(tq[0].reshape(-1), pad(fo.golomb_decode(rest[4:4 + t]), 27 * C))
        assert np.array_equal(q[0].reshape(-1), pad(fo.golomb_decode(rest[4 + t:]), N * C))


@pytest.mark.parametrize("N,C,bits,srate", [(256, 2, 16, 48000), (2048, 2, 8, 44100), (1792, 1, 24, 8000), (2048, 3, 12, 48000)])
def test_zero_lpc_decodes_like_profile1(be, N, C, bits, srate):
    rng = np.random.default_rng(N + C)
    F = 3
    ints = [rand_ints(rng, N, C) for _ in range(F)]
    q = np.stack([a[0] for a in ints]); tq = np.stack([a[1] for a in ints]); lpc = np.stack([a[2] for a in ints])
    got = be.digital(q, tq, lpc, N, C, bits, srate)
    want = be.p1_digital(q, tq, N, C, bits, srate)
    close(got, want, rel=1e-12)


def test_synth_matches_the_host_model(be):
    rng = np.random.default_rng(3)
    N, C = 512, 3
    mild = np.array([0, -7, 3, 1, 0, 0, -1, 0, 2, 0, 0, 0, 1])
    ints = [rand_ints(rng, N, C, np.stack([mild, np.roll(mild, 1) * (1 - 2 * (np.arange(13) % 2)), np.zeros(13)], 1)) for _ in range(2)]
    q = np.stack([a[0] for a in ints]); tq = np.stack([a[1] for a in ints]); lpc = np.stack([a[2] for a in ints])
    got = be.synth(q, tq, lpc, N, C, 14, 44100)
    for f in range(2):
        close(got[f], model_coeffs(q[f], tq[f], lpc[f], N, C, 14, 44100), rel=1e-12)


def test_filter_blow_up_falls_back_to_the_unfiltered_channel(be):
    rng = np.random.default_rng(5)
    N, C = 2048, 2
    lpc = np.zeros((13, C), np.int32)
    lpc[1, 0] = -30                                          # a1 = -2: y doubles every bin, far past 1e6 (and on to Inf / NaN)
    lpc[1, 1], lpc[2, 1] = -6, 2                             # a stable filter on the other channel
    q, tq, _ = rand_ints(rng, N, C)
    got = be.digital(q[None], tq[None], lpc[None], N, C, 16, 48000)[0]
    unf = be.digital(q[None], tq[None], np.zeros_like(lpc)[None], N, C, 16, 48000)[0]
    assert np.array_equal(got[:, 0], unf[:, 0])
    assert not np.allclose(got[:, 1], unf[:, 1])
    close(be.synth(q[None], tq[None], lpc[None], N, C, 16, 48000)[0], model_coeffs(q, tq, lpc, N, C, 16, 48000), rel=1e-12)


def test_inf_and_nan_coefficients_follow_the_host_model(be):
    """A huge threshold code makes (e/2)^quant(t) infinite: Inf and NaN (0 * Inf) coefficients, as in the host model; the
    inverse DCT then scrubs them to 0 (frad_hip.h: the documented deviation) and nothing raises."""
    rng = np.random.default_rng(9)
    N, C = 1024, 2
    q, tq, lpc = rand_ints(rng, N, C, np.stack([[0, -5, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], np.zeros(13)], 1))
    q[:20] = 0                                               # 0 * Inf = NaN below bin 20, +-Inf above
    tq[3, 0] = 2_000_000
    got = be.synth(q[None], tq[None], lpc[None], N, C, 10, 48000)[0]
    want = model_coeffs(q, tq, lpc, N, C, 10, 48000)
    assert np.isinf(want).any() and np.isnan(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    close(got[fin], want[fin], rel=1e-12)
    pcm = be.digital(q[None], tq[None], lpc[None], N, C, 10, 48000)[0]
    scrubbed = np.where(np.isfinite(want), want, 0.0)
    close(pcm, fo.idct_channels(scrubbed.T), rel=1e-9)


def test_corrupt_bodies_do_not_raise(be):
    rng = np.random.default_rng(13)
    N, C = 256, 2
    q, tq, lpc = rand_ints(rng, N, C, np.stack([[0, -5, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]] * 2, 1))
    good = model_body(lpc.reshape(-1), tq.reshape(-1), q.reshape(-1))
    n = int.from_bytes(good[:2], "big")
    truncated = good[:len(good) // 2]                        # the coefficient stream ends early: zero-filled (untrim)
    past_end = (len(good) + 100).to_bytes(2, "big") + good[2:]   # lpc_len past the end: the reference raises (struct.error)
    no_word = good[:2 + n + 2]                               # the '>I' word cut in half: the same
    bodies = [good, truncated, past_end, no_word, b"", b"\x00"]
    qq, tt, ll, st = be.ints(bodies, N, C)
    assert st.tolist() == [0, 0, 1, 1, 1, 1]
    assert np.array_equal(qq[0], q) and np.array_equal(tt[0], tq) and np.array_equal(ll[0], lpc)
    t = int.from_bytes(truncated[2 + n:6 + n], "big")
    part = fo.golomb_decode(truncated[6 + n + t:])
    assert np.array_equal(qq[1].reshape(-1), np.pad(part, (0, N * C - len(part)))) and np.array_equal(ll[1], lpc)
    for i in (2, 3, 4, 5):
        assert not qq[i].any() and not tt[i].any() and not ll[i].any()
    pcm = bridge_of(be).p2_decode_bodies(bodies, N, C, 16, 48000)
    assert np.isfinite(pcm).all() and not pcm[2:].any()


@pytest.mark.parametrize("C", [1, 3, 5])
def test_synth_across_wave_boundaries(be, C):
    """Lane = (frame, channel), 64 per wave: frames split between waves, and waves where one channel falls back"""
    rng = np.random.default_rng(17 + C)
    N, F = 256, 130 // C + 3
    q = rng.integers(-30, 31, (F, N, C)).astype(np.int32)
    tq = rng.integers(0, 40, (F, 27, C)).astype(np.int32)
    lpc = np.zeros((F, 13, C), np.int32)
    pick = rng.random((F, C))
    lpc[:, 1][pick < 0.7] = -6
    lpc[:, 2][pick < 0.7] = 2
    lpc[:, 12][pick < 0.4] = 1
    lpc[:, 1][pick < 0.1] = -30                              # blow-up: falls back inside a wave of filtered channels
    got = be.synth(q, tq, lpc, N, C, 20, 48000)
    for f in range(F):
        close(got[f], model_coeffs(q[f], tq[f], lpc[f], N, C, 20, 48000), rel=1e-12)
