"""Profile 2 (TNS) encoding (fourier/profile2.py:15-55, tools/p2tools.py:55-103) against the reference's own outputs
(g8_p2_enc.npz, written by tools/gen_golden_p2_enc.py) and a host model.  "emu": the CPU interpreter of the same kernel source
(frad_p2_analogue, frad_p2_golomb_encode); "gpu": the MI355X through core and HipBridge."""
import random

import numpy as np
import pytest
from scipy.fft import dct

from conftest import load_npz
from frad_python_amd import Decoder, Encoder
from frad_python_amd.backend.pcmformat import pcm_dtype_code
from test_p2_decode import EmuP2Bridge

P2_DEPTHS = (8, 10, 12, 14, 16, 20, 24)


# --------------------------------------------------------------------------------------------------------- backends
class EmuP2Enc(EmuP2Bridge):
    """The encoder's and the decoder's bridge interface for profile 2 on the CPU interpreter build."""

    def analogue(self, raw: bytes, fmt, n, N, C, bits, srate, loss, hop=None, n_valid=None):
        hop = N if hop is None else hop
        nv = N if n_valid is None else n_valid
        buf = np.frombuffer(raw + bytes(16), np.uint8).copy()
        q = np.full((max(n, 1), N, C), -7, np.int32); tq = np.full((max(n, 1), 27, C), -7, np.int32)
        lpc = np.full((max(n, 1), 13, C), -7, np.int32)
        self.lib.p2_analogue(buf.ctypes.data, pcm_dtype_code(fmt), n, N, C, hop, nv, bits, srate, float(loss), 2,
                             q.ctypes.data, tq.ctypes.data, lpc.ctypes.data)
        return q[:n], tq[:n], lpc[:n]

    def bodies(self, q, tq, lpc):
        n, N, C = q.shape
        stride = self.lib.p2_golomb_bound(N, C)
        rows = np.zeros((max(n, 1), stride), np.uint8); nb = np.zeros(max(n, 1), np.int64)
        q, tq, lpc = (np.ascontiguousarray(a, np.int32) for a in (q, tq, lpc))
        self.lib.p2_golomb_encode(q.ctypes.data, tq.ctypes.data, lpc.ctypes.data, n, N, C, rows.ctypes.data, stride, nb.ctypes.data)
        return [rows[i, :nb[i]].tobytes() for i in range(n)]

    def p2_encode_bodies(self, pcm, fmt, n_frames, N, C, bits, srate, loss_level, hop, n_valid, raw_be_ints=True):
        return self.bodies(*self.analogue(pcm, fmt, n_frames, N, C, bits, srate, loss_level, hop, n_valid))


class GpuP2Enc:
    def __init__(self):
        import torch
        from frad_python_amd import core
        from frad_python_amd.bridge import HipBridge
        self.t, self.core, self.bridge = torch, core, HipBridge()
        self.dev = self.bridge.device

    def analogue(self, raw, fmt, n, N, C, bits, srate, loss, hop=None, n_valid=None):
        pcm = self.t.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(self.dev)
        return tuple(a.cpu().numpy() for a in self.core.p2_analogue_batch(pcm, fmt, n, N, C, bits, srate, loss,
                                                                          frame_stride=hop, n_valid=n_valid))

    def bodies(self, q, tq, lpc):
        d = lambda a: self.t.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.dev)
        flat, off = self.core.p2_golomb_encode_batch(d(q), d(tq), d(lpc))
        flat, off = flat.cpu().numpy().tobytes(), off.cpu().numpy()
        return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def be(request):
    return EmuP2Enc() if request.param == "emu" else GpuP2Enc()


def bridge_of(be):
    return be if isinstance(be, EmuP2Enc) else be.bridge


@pytest.fixture(scope="module")
def g8():
    return load_npz("g8_p2_enc.npz")


def part(d, name, i):
    return d[name][d[name + "_off"][i]:d[name + "_off"][i + 1]]


def frames_of(d):
    fmts = [str(f) for f in d["formats"]]
    for i, (N, C, bits, srate, fi, step, loss) in enumerate(d["meta"].tolist()):
        yield dict(N=N, C=C, bits=bits, srate=srate, fmt=fmts[fi], step=step, loss=loss / 1000, raw=part(d, "raw", i).tobytes(),
                   body=part(d, "body", i).tobytes(), q=part(d, "q", i).reshape(N, C), tq=part(d, "tq", i).reshape(27, C),
                   lpc=part(d, "lpc", i).reshape(13, C), pcm=part(d, "pcm", i).reshape(-1, C))


def streams_of(d):
    fmts = [str(f) for f in d["formats"]]
    for i, (ratio, bits, fsize, srate, C, fi, rows) in enumerate(d["stream_meta"].tolist()):
        yield dict(ratio=ratio, bits=bits, fsize=fsize, srate=srate, C=C, fmt=fmts[fi], stream=part(d, "stream", i).tobytes(),
                   raw=part(d, "stream_raw", i).tobytes(), pcm=part(d, "stream_pcm", i).reshape(rows, C))


def psnr(a, ref):
    err = np.max(np.abs(a - ref))
    return np.inf if err == 0 else 20 * np.log10(max(np.max(np.abs(ref)), 1e-300) / err)


# --------------------------------------------------------------------------------------------------------- per-frame parity
def test_frames_match_the_reference(be, g8):
    """Today's failure: frad_p2_analogue / core.p2_analogue_batch do not exist."""
    lpc_bad = tq_bad = q_off = q_total = tns = 0
    for fr in frames_of(g8):
        q, tq, lpc = be.analogue(fr["raw"], fr["fmt"], 1, fr["N"], fr["C"], fr["bits"], fr["srate"], fr["loss"])
        lpc_bad += int(np.sum(lpc[0] != fr["lpc"])); tq_bad += int(np.sum(tq[0] != fr["tq"]))
        assert np.all(lpc[0, 0] == 0)
        dq = np.abs(q[0].astype(np.int64) - fr["q"])
        assert dq.max() <= 1, (fr["N"], fr["C"], fr["fmt"])
        q_off += int(np.sum(dq != 0)); q_total += dq.size
        tns += bool(np.any(fr["lpc"]))
        if np.array_equal(q[0], fr["q"]) and np.array_equal(tq[0], fr["tq"]) and np.array_equal(lpc[0], fr["lpc"]):
            assert be.bodies(q, tq, lpc)[0] == fr["body"]
    print(f"\nprofile-2 encode parity: {len(g8['meta'])} frames ({tns} TNS), lpc mismatches {lpc_bad}, tq mismatches {tq_bad}, "
          f"q off by one {q_off} of {q_total}")
    assert lpc_bad == 0 and tq_bad == 0
    assert q_off <= 1e-3 * q_total


def test_bodies_round_trip_through_the_device_decoder(be, g8):
    worst = np.inf
    br = bridge_of(be)
    for fr in frames_of(g8):
        N, C = fr["N"], fr["C"]
        ints = be.analogue(fr["raw"], fr["fmt"], 1, N, C, fr["bits"], fr["srate"], fr["loss"])
        body = be.bodies(*ints)[0]
        pcm = br.p2_decode_bodies([body], N, C, fr["bits"], fr["srate"])[0]
        p = psnr(pcm[::fr["step"]], fr["pcm"])
        worst = min(worst, p)
        assert p > 100, (N, C, fr["fmt"], p)
    print(f"\nworst round-trip PSNR against the reference decode: {worst:.1f} dB")


# --------------------------------------------------------------------------------------------------------- whole streams
def encode(br, s, cuts=()):
    enc = Encoder(2, s["srate"], s["C"], s["bits"], s["fsize"], s["fmt"], bridge=br, allow_profile2=True)
    enc.set_overlap_ratio(s["ratio"])
    enc.set_loss_level(0.5)
    out, last = [], 0
    for c in list(cuts) + [len(s["raw"])]:
        out.append(enc.process(s["raw"][last:c]).buf)
        last = c
    out.append(enc.flush().buf)
    return b"".join(out)


def test_streams_match_the_reference(be, g8):
    for s in streams_of(g8):
        assert encode(bridge_of(be), s) == s["stream"], s["ratio"]


def test_streams_are_split_invariant(be, g8):
    rng = random.Random(7)
    for s in streams_of(g8):
        cuts = sorted(rng.sample(range(1, len(s["raw"])), 5))
        assert encode(bridge_of(be), s, cuts) == s["stream"], (s["ratio"], cuts)


def test_streams_decode_like_the_reference(be, g8):
    for s in streams_of(g8):
        out = encode(bridge_of(be), s)
        dec = Decoder(bridge=bridge_of(be))
        pcm = np.concatenate([p.reshape(-1, s["C"]) for p in (dec.process(out).pcm, dec.flush().pcm) if p.size])
        assert pcm.shape == s["pcm"].shape
        assert psnr(pcm, s["pcm"]) > 100


def test_little_endian_flag_is_ignored_by_profile2(be, g8):
    s = next(streams_of(g8))
    enc = Encoder(2, s["srate"], s["C"], s["bits"], s["fsize"], s["fmt"], bridge=bridge_of(be), allow_profile2=True)
    enc.set_overlap_ratio(s["ratio"]); enc.set_loss_level(0.5); enc.set_little_endian(True)
    out = enc.process(s["raw"]).buf + enc.flush().buf
    assert out[:64] == s["stream"][:64] or len(out) == len(s["stream"])


def _encode_pcm(be, raw, fmt, C=2, fsize=512):
    enc = Encoder(2, 48000, C, 24, fsize, fmt, bridge=bridge_of(be), allow_profile2=True)
    return enc.process(raw).buf + enc.flush().buf


def _decode_pcm(be, out, C=2):
    dec = Decoder(bridge=bridge_of(be))
    return np.concatenate([p.reshape(-1, C) for p in (dec.process(out).pcm, dec.flush().pcm) if p.size])


def _sparse_signal(n=3 * 512 + 77, C=2):
    rng = np.random.default_rng(3)
    return np.clip(rng.normal(0, 0.2, (n, C)) * (rng.random((n, 1)) < 0.05), -0.99, 0.99)


@pytest.mark.parametrize("fmt", ["u8", "s16le", "u32le", "s64le", "f16le", "f32le", "f64be"])
def test_every_pcm_format_round_trips(be, fmt):
    from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64
    x = _sparse_signal()
    raw = from_f64(x, fmt).astype(ff_format_to_numpy_type(fmt)).tobytes()
    pcm = _decode_pcm(be, _encode_pcm(be, raw, fmt))
    assert len(pcm) >= len(x)                                  # the flushed frame decodes at its compact size, as upstream's
    assert np.max(np.abs(pcm[:len(x)] - x)) < 0.05


@pytest.mark.parametrize("fmt,dt", [("s16be", ">i2"), ("s32be", ">i4")])
def test_big_endian_ints_keep_the_reference_quirk(be, fmt, dt):
    """upstream's to_f64 does not normalise big-endian integers (pcmformat.py:37-45): the stream is that of their raw values"""
    v = np.round(_sparse_signal() * 30000)
    assert _encode_pcm(be, v.astype(dt).tobytes(), fmt) == _encode_pcm(be, v.astype("<f8").tobytes(), "f64le")


# --------------------------------------------------------------------------------------------------------- host model
def host_tns(m: np.ndarray):
    """tns_analysis as the reference documents it (p2tools.py): -> (coefficients to quantise, 13 LPC integers, reason)"""
    zero = np.zeros(13, np.int64)
    n = len(m)
    if n < 24:
        return m, zero, "short"
    with np.errstate(all="ignore"):
        if not np.exp(np.mean(np.log(np.abs(m) + 1e-10))) / (np.mean(np.abs(m)) + 1e-10) < 0.5:
            return m, zero, "flat"
        if np.sum(m * m) < 1e-10:
            return m, zero, "silent"
        s = m - m.mean()
        nrm = np.sqrt(np.sum(s * s))
        if nrm > 1e-6:
            s = s / nrm
        r = np.array([np.dot(s[:n - k], s[k:]) for k in range(13)]) * np.exp(-0.5 * (np.arange(13) * 0.01) ** 2)
    a = np.zeros(13); a[0] = 1.0
    err = r[0]
    if err > 1e-10:
        for i in range(1, 13):
            k = -np.dot(a[:i], r[i:0:-1]) / err
            k = float(np.clip(k, -0.96, 0.96)) if abs(k) >= 0.96 else k
            a[1:i] = a[1:i] + k * a[i - 1:0:-1]
            a[i] = k
            err *= 1 - k * k
            if err <= 1e-12:
                break
    if np.sum(np.abs(a[1:])) < 0.01:
        return m, zero, "weak"
    lq = np.zeros(13, np.int64)
    lq[1:] = np.round(np.clip(a[1:] * 15, -15, 14))
    if not lq.any():
        return m, zero, "weak"
    b = np.r_[1.0, lq[1:] / 15]
    res = np.convolve(b, m)[:n]
    if not np.all(np.isfinite(res)) or np.max(np.abs(res)) > 1e6:
        return m, zero, "blowup"
    oe, re = np.sum((m - m.mean()) ** 2), np.sum((res - res.mean()) ** 2)
    gain = 0 if (oe < 1e-10 or re < 1e-10 or re >= oe) else 20 * np.log10(oe / re)
    if gain < np.log10(2) / 10:
        return m, zero, "gain"
    return res, lq, "tns"


BANDS_HZ = (0, 200, 400, 600, 800, 1000, 1200, 1400, 1600, 2000, 2400, 2800, 3200, 4000, 4800, 5600, 6800, 8000, 9600, 12000,
            15600, 20000, 24000, 28800, 34400, 40800, 48000, 2 ** 32 - 1)


def host_masked(x: np.ndarray, bits: int, srate: int, loss: float) -> np.ndarray:
    """the masked spectrum of one channel (profile2.py:24-31 with p1tools' thresholds and ramp)"""
    N = len(x)
    X = dct(x, norm="forward")
    edge = [min(round(N / (srate / 2) * f), N) for f in BANDS_HZ]
    thr = np.zeros(27)
    for i in range(27):
        seg = np.abs(X[edge[i]:edge[i + 1]] * 2.0 ** (bits - 1))
        if len(seg) == 0:
            break
        fk = (BANDS_HZ[i] + BANDS_HZ[i + 1]) / 2000
        ath = 10 ** ((3.64 * fk ** -0.8 - 6.5 * np.exp(-0.6 * (fk - 3.3) ** 2) + 1e-3 * fk ** 4) / 20)
        thr[i] = max(np.sqrt(np.mean(seg ** 2)) ** 0.8, min(ath, 1.0)) * max(abs(loss), 0.125)
    div = np.zeros(N)
    for i in range(26):
        div[edge[i]:edge[i + 1]] = np.linspace(thr[i], thr[i + 1], edge[i + 1] - edge[i], endpoint=False)
    with np.errstate(all="ignore"):
        return X / np.where(div == 0, np.inf, div)


def run_frame(be, x, bits=16, srate=48000, loss=0.5, n_valid=None):
    x = np.ascontiguousarray(x, "<f8")
    N, C = x.shape
    return be.analogue(x.tobytes(), "f64le", 1, N, C, bits, srate, loss, n_valid=n_valid)


def check_against_model(be, x, expect, bits=16):
    q, tq, lpc = run_frame(be, x, bits)
    for c in range(x.shape[1]):
        coef, lq, why = host_tns(host_masked(x[:, c], bits, 48000, 0.5))
        assert why in expect, why
        assert np.array_equal(lpc[0, :, c], lq), why
        with np.errstate(all="ignore"):
            y = coef * 2.0 ** (bits - 1)
            ref = np.sign(y) * np.abs(y) ** 0.75
        ok = np.isfinite(ref)
        assert np.all(np.abs(q[0, ok, c] - np.round(ref[ok])) <= 1)
    return q, lpc


def test_silence_keeps_the_masked_spectrum(be):
    q, lpc = check_against_model(be, np.zeros((2048, 2)), {"flat", "silent"})
    assert not q.any() and not lpc.any()


def test_short_flush_frame_never_takes_tns(be):
    x = np.zeros((128, 1)); x[3, 0] = 0.9; x[9, 0] = -0.5
    q, tq, lpc = run_frame(be, x, n_valid=20)
    q2, tq2, lpc2 = run_frame(be, np.r_[x[:20], np.zeros((108, 1))])
    assert np.array_equal(q, q2) and np.array_equal(tq, tq2) and np.array_equal(lpc, lpc2)


def test_click_frame_takes_tns_like_the_model(be):
    x = np.zeros((2048, 1)); x[100, 0] = 0.8; x[1500, 0] = -0.4
    q, lpc = check_against_model(be, x, {"tns"})
    assert lpc.any()


def test_blowup_rejects_the_residual(be):
    """a spectrum so large that the residual exceeds 1e6: the masked spectrum is kept and the LPC is zero"""
    x = np.zeros((2048, 1)); x[100, 0] = 1e35; x[1500, 0] = -4e34
    q, lpc = check_against_model(be, x, {"blowup"}, bits=8)
    assert not lpc.any()


def test_nan_and_inf_input_give_zero_lpc(be):
    x = np.zeros((1024, 2)); x[5, 0] = np.nan; x[7, 1] = np.inf; x[300, :] = 0.5
    q, tq, lpc = run_frame(be, x)
    assert not lpc.any()


# --------------------------------------------------------------------------------------------------------- refusals
def test_encoder_still_refuses_profile2_without_the_flag():
    with pytest.raises(SystemExit):
        Encoder(2, 48000, 2, 16, 2048, "s16le")
    with pytest.raises(SystemExit):
        Encoder(2, 48000, 2, 16, 2048, "s16le", allow_profile2=False)
    assert Encoder.verify_profile(2) is not None
    e = Encoder(1, 48000, 2, 16, 2048, "s16le")
    assert e.set_profile(2, 48000, 2, 16, 2048) is not None and e.get_profile() == 1


def test_opt_in_admits_profile2_and_keeps_ecc_refused():
    e = Encoder(2, 48000, 2, 16, 2048, "s16le", allow_profile2=True)
    assert e.get_profile() == 2
    assert not isinstance(e.set_profile(1, 48000, 2, 16, 2048), str) and e.get_profile() == 1
    assert not isinstance(e.set_profile(2, 48000, 2, 16, 2048), str) and e.get_profile() == 2
    with pytest.raises(NotImplementedError):
        e.set_ecc(True, (96, 24))


def test_wrappers_validate_before_launch():
    import torch
    from frad_python_amd import core
    t = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        core.p2_analogue_batch(t, "s16le", 1, 128, 1, 9, 48000, 0.5)      # not a profile-2 depth
    with pytest.raises(ValueError):
        core.p2_analogue_batch(t, "s16le", 1, 128, 65, 16, 48000, 0.5)    # more than 64 channels
    with pytest.raises(ValueError):
        core.p2_analogue_batch(t, "s16le", 1, 128, 1, 16, 48000, 0.5)     # 16 bytes of PCM for a frame of 256
    with pytest.raises(ValueError):
        core.p2_golomb_encode_batch(torch.zeros((1, 128, 1), dtype=torch.int32), torch.zeros((1, 27, 1), dtype=torch.int32),
                                    torch.zeros((1, 12, 1), dtype=torch.int32))


# --------------------------------------------------------------------------------------------------------- cfg-2 scale
@pytest.mark.gpu
def test_cfg2_sized_batch_round_trips_on_the_device():
    """about 15 000 stereo frames of 2048 through frad_p2_analogue, the coder, and the device decoder back"""
    import torch
    from frad_python_amd import core
    n, N, C = 15000, 2048, 2
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((n * N, C), generator=g) * 3000 * (torch.rand((n * N, 1), generator=g) < 0.01)).clamp(-32767, 32767)
    pcm = x.to(torch.int16).cuda().view(torch.uint8).reshape(-1)
    q, tq, lpc = core.p2_analogue_batch(pcm, "s16le", n, N, C, 16, 48000, 0.5)
    assert int((lpc != 0).any(dim=1).any(dim=1).sum()) > n // 2
    flat, off = core.p2_golomb_encode_batch(q, tq, lpc)
    none, off0 = core.p2_golomb_encode_batch(q[:0], tq[:0], lpc[:0])      # an empty batch: no bytes and the one offset
    assert none.dtype == torch.uint8 and none.numel() == 0 and off0.dtype == torch.int64 and off0.numel() == 1
    flat_s = torch.cat([flat, torch.zeros(16, dtype=torch.uint8, device=flat.device)])
    q2, tq2, lpc2, st = core.p2_golomb_decode_batch(flat_s, off, N, C)
    assert torch.equal(q, q2) and torch.equal(tq, tq2) and torch.equal(lpc, lpc2) and not st.any()
    out = core.p2_digital_batch(q2, tq2, lpc2, N, C, 16, 48000).cpu().numpy()
    # sampled frames against the CPU interpreter of the same source: the integers exactly, the decoded PCM to 1e-9 (a fixed
    # PCM bound would not do: at loss level 0.5 this signal is coded lossily, and the reference itself is off by ~0.15)
    emu = EmuP2Enc()
    raw = pcm.cpu().numpy().tobytes()
    for f in (0, 1, 777, 7499, 14998, 14999):
        fr = raw[f * N * C * 2:(f + 1) * N * C * 2]
        eq, etq, elpc = emu.analogue(fr, "s16le", 1, N, C, 16, 48000, 0.5)
        assert np.array_equal(eq[0], q[f].cpu().numpy()) and np.array_equal(etq[0], tq[f].cpu().numpy())
        assert np.array_equal(elpc[0], lpc[f].cpu().numpy())
        ref = emu.digital(eq, etq, elpc, N, C, 16, 48000)[0]
        assert np.max(np.abs(out[f] - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref))), f
