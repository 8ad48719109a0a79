"""Profile 1 decoder (K8, frad_p1_digital: dequantise, spread the 27 band thresholds, inverse DCT) at every depth, rate, compact
size and table edge, against a long-double model and a derived bound; the overlap-add behind it against a numpy model, bitwise.

The model (``model_decode``) works in ``np.longdouble`` and uses neither scipy nor the oracle's power function.  For one
frame q [N, C], tq [27, C]:

    f  = sign(q) |q|^(4/3) / 2^(bits-1)                      bits not a profile-1 depth -> 16 (profile1.py:16)
    t  = (e/2)^(sign(tq) |tq|^0.75)                           e/2 is the reference's double ``np.e / 2``, widened
    sp = 0; for bands i = 0 .. 25 with b > a (edges of fo.band_edges at the snapped rate, clipped to N):
         sp[a:b] = t[i] + arange(b - a) * ((t[i+1] - t[i]) / (b - a))
    X  = f * sp
    x[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)     the angle (2n+1) k mod 4N reduced as an integer first

The bound, with u = 2^-53, per frame and channel, T = the largest |tq| of that frame and channel, X the model's:

    |got - model| <= u (8 + T^0.75 + 8 log2 N) sum_k |X_k|

  * 8 log2 N: the project's FFT constant (test_parity.py: 8 eps log2 N max|X| for the forward transform), applied to sum |X|
    because an inverse DCT sums every bin into every sample;
  * 8: per coefficient -- cbrt, two products, the ramp's two roundings and the threshold's pow;
  * T^0.75: the rounding of the exponent y = |tq|^0.75 amplified by (e/2)^y: y ln(e/2) = 0.307 y, times about 3 ulp for
    sqrt * sqrt(sqrt) against pow.

The model is used up to N = 2048.  Above it the reference is ``fo.p1_digital_post`` and the tolerance 1.5 x the bound: the
oracle itself stays within 0.5 of it (``test_bound_separates_float64_from_less``, which also shows that a model whose thresholds
are rounded to float32 misses the bound by five orders of magnitude and more: the bound tells float64 from anything less).
The older decode assertions, 1e-12 * max(1, max|ref|), are 20 to 180 times looser on the depth and rate cases below.

Every test prints ``worst |got - model| / bound``.  Observed maxima, emulator (x86-64, glibc) / MI355X:
    oracle against the model (no device)   0.091 over the 56 depth and rate cases
    depths (and converted output)          0.208 / 0.213
    rates                                  0.094 / 0.094
    every compact size                     0.229 / 0.241  (N > 2048, against the oracle: 0.052 / 0.057 of the bound, limit 1.5)
    frames per block, band geometry        0.221 / 0.221
    table edges, zero frames               0.176 / 0.176
    batches                                0.369 / 0.355
    float32 thresholds in the model        5e5 to 2e6

The overlap-add is held to the numpy model of decoder.py:28-46 bit for bit.  On the MI355X that failed at first: the kernels
evaluated the Hann ramp with the device's cos, which differs from the host's in the last bit for about one argument in 500
(2577 of 1 152 000 samples of the 300-frame case were one ulp off, none on the emulator).  The kernels now read the ramp from a
table the host computes (``hann_table``, csrc/frad_p1.hip), and both legs give the model's samples.

Routes of ``p1_digital_out`` (csrc/frad_p1.hip), as the case ids name them: ``wave`` the table-driven wave kernel (N = 2048, one or
two channels), ``wave+redo`` with k_p1_inv_redo behind it for the frames it marks, ``inv`` k_p1_inv<LOG2M, 256 | 1024>, ``grp``
k_p1_inv_grp, ``mixed`` the mixed-radix kernel, ``direct`` k_p1_inv_direct, ``workspace`` the HBM-workspace route.  ``_route``
mirrors the host dispatch to name them; which frames leave the wave kernel's tables is asserted from the integers.
"""
import functools
import hashlib

import numpy as np
import pytest

from helpers import EmuBackend, GpuBackend
from frad_python_amd import synth
from oracle import frad_oracle as fo

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the model needs a long double wider than float64"
U = 2.0 ** -53
HALF_E = LD(np.e / 2)
MODEL_MAX_N = 2048
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

_backends = {}
_observed = {}


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param not in _backends:
        _backends[request.param] = EmuBackend() if request.param == "emu" else GpuBackend()
    return _backends[request.param]


def _legs(cases, emu=lambda *case: True):
    """(backend, case...) parameters for ``be`` given indirectly: the gpu leg runs every case, the emu leg those ``emu`` admits"""
    out = []
    for case in cases:
        cid = case[0]
        if emu(*case[1:]):
            out.append(pytest.param("emu", *case[1:], id=f"emu-{cid}"))
        out.append(pytest.param("gpu", *case[1:], id=f"gpu-{cid}", marks=pytest.mark.gpu))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the model and the bound
# ---------------------------------------------------------------------------------------------------------------------
def _depth(bits):
    return bits if bits in fo.P1_DEPTHS else 16


def clipped_edges(N, srate):
    return [min(e, N) for e in fo.band_edges(N, fo.compact_valid_srate(srate))]


def model_spectrum(q, tq, bits, srate, t_dtype=None):
    """q [F, N, C], tq [F, 27, C] -> X [F, N, C] in long double; ``t_dtype``: round the thresholds to that type (a defect to detect)"""
    F, N, C = q.shape
    qi, ti = q.astype(np.int64), tq.astype(np.int64)
    f = np.sign(qi) * np.abs(qi).astype(LD) ** (LD(4) / LD(3)) / LD(2) ** (_depth(bits) - 1)
    t = HALF_E ** (np.sign(ti) * np.abs(ti).astype(LD) ** LD(0.75))
    if t_dtype is not None:
        t = t.astype(t_dtype).astype(LD)
    edges = clipped_edges(N, srate)
    sp = np.zeros((F, N, C), LD)
    for i in range(fo.N_BANDS - 1):
        a, b = edges[i], edges[i + 1]
        if b > a:
            step = (t[:, i + 1] - t[:, i]) / LD(b - a)
            sp[:, a:b] = t[:, i, None, :] + np.arange(b - a, dtype=LD)[None, :, None] * step[:, None, :]
    return f * sp


@functools.lru_cache(maxsize=2)
def _cos_matrix(N):
    """[n, k] -> cos(pi k (2n+1) / 2N), doubled for k >= 1: the angle is reduced mod 4N as an integer, then scaled"""
    pi = 4 * np.arctan(LD(1))
    tab = np.cos(pi * np.arange(4 * N, dtype=LD) / LD(2 * N))
    n = np.arange(N, dtype=np.int64)
    m = tab[((2 * n[:, None] + 1) * n[None, :]) % (4 * N)]
    m[:, 1:] *= 2
    return m


def model_decode(q, tq, bits, srate, t_dtype=None):
    """-> (x [F, N, C], X [F, N, C]), long double"""
    X = model_spectrum(q, tq, bits, srate, t_dtype)
    F, N, C = X.shape
    x = _cos_matrix(N) @ np.ascontiguousarray(X.transpose(1, 0, 2)).reshape(N, F * C)
    return x.reshape(N, F, C).transpose(1, 0, 2), X


def bound_of(X, tq):
    """[F, C]: u (8 + T^0.75 + 8 log2 N) sum |X|"""
    N = X.shape[1]
    T = np.abs(tq.astype(np.int64)).max(axis=1).astype(LD)
    return LD(U) * (8 + T ** LD(0.75) + 8 * np.log2(LD(N))) * np.abs(X).sum(axis=1)


def oracle_decode(q, tq, bits, srate):
    F, N, C = q.shape
    fb, sr = fo.P1_DEPTHS.index(_depth(bits)), fo.compact_valid_srate(srate)
    return np.stack([fo.p1_digital_post(q[f].reshape(-1), tq[f].reshape(-1), fb, C, sr, N) for f in range(F)])


_refs = {}


def reference(q, tq, bits, srate):
    """-> (reference [F, N, C], bound [F, C], tolerance in bounds); computed once per case and shared by the legs"""
    key = (hashlib.sha1(q.tobytes()).digest(), hashlib.sha1(tq.tobytes()).digest(), q.shape, _depth(bits), fo.compact_valid_srate(srate))
    if key not in _refs:
        if q.shape[1] <= MODEL_MAX_N:
            x, X = model_decode(q, tq, bits, srate)
            _refs[key] = (x, bound_of(X, tq), 1.0)
        else:
            _refs[key] = (oracle_decode(q, tq, bits, srate), bound_of(model_spectrum(q, tq, bits, srate), tq), 1.5)
        for a in _refs[key][:2]:
            a.setflags(write=False)
    return _refs[key]


def worst_ratio(got, ref, bound):
    """max over frames and channels of max_n |got - ref| / bound; where the bound is 0 (a silent channel) only 0 error passes"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref).max(axis=1)
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(r))


def check(be, q, tq, bits, srate, what, group):
    """decode on ``be`` and hold every element against the reference; -> the decoded frames"""
    F, N, C = q.shape
    got = be.p1_digital(q, tq, N, C, bits, srate)
    ref, bound, tol = reference(q, tq, bits, srate)
    r = worst_ratio(got, ref, bound)
    key = (be.name, group, tol)                                # (tol 1.5: against the oracle)
    _observed[key] = max(_observed.get(key, 0.0), r)
    print(f"[p1 decode] {be.name} {what}: worst |got - model| / bound = {r:.3f} (limit {tol}; {group} so far {_observed[key]:.3f})")
    assert r <= tol, f"{what}: |got - model| reaches {r:.3f} of the bound (limit {tol})"
    return got


# ---------------------------------------------------------------------------------------------------------------------
# inputs: the oracle's own integers of a harmonic mix, s16le
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ints(N, C, F, bits=16, srate=48000):
    """-> (q int32 [F, N, C], tq int32 [F, 27, C]) of ``fo.p1_analogue_pre`` at loss level 1, read-only"""
    raw = synth.to_pcm(synth.harmonic_mix(F * N, C, srate, seed=7), "s16le")
    dt = fo.pcm_dtype("s16le")
    q, tq = np.empty((F, N, C), np.int64), np.empty((F, fo.N_BANDS, C), np.int64)
    for f in range(F):
        a, b, _ = fo.p1_analogue_pre(fo.to_f64(raw[f * N:(f + 1) * N], dt), bits, srate, 1.0)
        q[f], tq[f] = a.reshape(N, C), b.reshape(fo.N_BANDS, C)
    assert np.abs(q).max() <= INT32_MAX and np.abs(tq).max() <= INT32_MAX
    q, tq = q.astype(np.int32), tq.astype(np.int32)
    q.setflags(write=False); tq.setflags(write=False)
    return q, tq


def marked(q, tq):
    """[F] bool: the frames that leave the wave kernel's tables (|q| >= 256 or a band code outside [0, 256))"""
    return (np.abs(q.astype(np.int64)) >= 256).any(axis=(1, 2)) | ((tq < 0) | (tq >= 256)).any(axis=(1, 2))


def _scratch_bytes(cfs, N):
    return cfs * fo.N_BANDS * 16 + 28 * 8 + 32 * 4 + (N + 15) // 16 * 16


def _route(N, C, leaves=False):
    """the kernel family ``p1_digital_out`` gives this geometry (a mirror of the host dispatch, for the case ids)"""
    lds = 160 * 1024
    if N & (N - 1) == 0:
        if N == 2048 and C <= 2:
            return "wave+redo" if leaves else "wave"
        team = {6: 16, 7: 32, 8: 64, 9: 64, 10: 64, 11: 128, 12: 256, 13: 512}[N.bit_length() - 2]
        whole = C * team <= 1024 and C * (N // 2) * 16 + _scratch_bytes(C, N) <= lds
        return ("inv1024" if C * team > 256 else "inv256") if whole else "grp"
    P = [N // 2 // r for r in (3, 5, 7) if N // 2 % r == 0 and (N // 2 // r) & (N // 2 // r - 1) == 0]
    if P and 64 <= P[0] <= 1024 and 2 * N * 8 + _scratch_bytes(1, N) <= lds:
        return "mixed"
    return "direct" if 2 * N * C * 8 + _scratch_bytes(C, N) <= lds else "workspace"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the bound itself, without a device
# ---------------------------------------------------------------------------------------------------------------------
DEPTHS = [8, 12, 16, 24, 32, 48, 64, 20]                          # 20: not a profile-1 depth, decoded as 16 (p1_scale_bits)
DEPTH_GEOMS = [(2048, 2, 2), (2048, 1, 3), (512, 2, 2), (640, 1, 2)]                       # (N, C, F)
RATE_GEOMS = [(2048, 2, 2), (256, 1, 2)]
MODEL_GRID = ([(N, C, F, b, 48000) for (N, C, F) in DEPTH_GEOMS for b in DEPTHS] +
              [(N, C, F, 16, r) for (N, C, F) in RATE_GEOMS for r in fo.COMPACT_SRATES])


def _leaves_tables(C, F, bits):
    """the frames of the N = 2048 depth cases whose s16le integers leave the wave kernel's tables: all of them from 32 bit on
    (|q| to 299 .. 25 608, codes to 507), at 24 bit the first mono frame alone (|q| = 400), its neighbour in the wave not"""
    return tuple(range(F)) if bits in (32, 48, 64) else (0,) if (C, bits) == (1, 24) else ()


def test_bound_separates_float64_from_less():
    """The oracle (float64 numpy + pocketfft) stays within half the bound on every depth and rate case that uses the model; the
    model with its thresholds rounded to float32 misses the bound on each of a sample of them."""
    worst = 0.0
    for (N, C, F, bits, srate) in MODEL_GRID:
        q, tq = _ints(N, C, F, bits, srate)
        ref, bound, tol = reference(q, tq, bits, srate)
        r = worst_ratio(oracle_decode(q, tq, bits, srate), ref, bound)
        worst = max(worst, r)
        assert tol == 1.0 and r <= 0.5, f"N={N} C={C} bits={bits} {srate} Hz: the oracle uses {r:.3f} of the bound"
    print(f"[p1 decode] the oracle against the model: worst |oracle - model| / bound = {worst:.3f} over {len(MODEL_GRID)} cases")
    for (N, C, F, bits, srate) in [(2048, 2, 2, 16, 48000), (2048, 1, 3, 64, 48000), (512, 2, 2, 8, 48000), (640, 1, 2, 24, 48000),
                                   (256, 1, 2, 16, 8000), (256, 1, 2, 16, 96000)]:
        q, tq = _ints(N, C, F, bits, srate)
        ref, bound, _ = reference(q, tq, bits, srate)
        assert np.abs(tq).max() >= 2, "float32 holds (e/2)^0 and (e/2)^1 as well as float64 does"
        r32 = worst_ratio(np.asarray(model_decode(q, tq, bits, srate, np.float32)[0], np.float64), ref, bound)
        print(f"[p1 decode] float32 thresholds, N={N} C={C} bits={bits} {srate} Hz: {r32:.3g} of the bound")
        assert r32 > 1.0, f"N={N} C={C} bits={bits}: float32 thresholds pass the bound ({r32:.3f})"


# ---------------------------------------------------------------------------------------------------------------------
# 2. depth
# ---------------------------------------------------------------------------------------------------------------------
def _depth_cases():
    return [pytest.param(N, C, F, b, id=f"{_route(N, C, bool(_leaves_tables(C, F, b)))}-{N}x{C}-bits{b}") for (N, C, F) in DEPTH_GEOMS for b in DEPTHS]


@pytest.mark.parametrize("N,C,F,bits", _depth_cases())
def test_every_depth(be, N, C, F, bits):
    q, tq = _ints(N, C, F, bits)
    if N == 2048:                                              # or a case silently stops reaching its route
        assert tuple(np.flatnonzero(marked(q, tq))) == _leaves_tables(C, F, bits), "other frames leave the tables than the case id says"
    got = check(be, q, tq, bits, 48000, f"{N}x{C} bits {bits}", "depths")
    if bits == 20:
        q16, tq16 = _ints(N, C, F, 16)
        assert np.array_equal(q, q16) and np.array_equal(tq, tq16)
        assert got.tobytes() == be.p1_digital(q, tq, N, C, 16, 48000).tobytes(), "an unknown depth is not decoded as 16 bit"


# ---------------------------------------------------------------------------------------------------------------------
# 3. rate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srate", fo.COMPACT_SRATES)
@pytest.mark.parametrize("N,C,F", [pytest.param(*g, id=f"{_route(g[0], g[1])}-{g[0]}x{g[1]}") for g in RATE_GEOMS])
def test_every_table_rate(be, N, C, F, srate):
    q, tq = _ints(N, C, F, 16, srate)
    if N == 2048:
        assert not marked(q, tq).any()
    check(be, q, tq, 16, srate, f"{N}x{C} {srate} Hz", "rates")


@pytest.mark.parametrize("srate,snapped", [(50000, 64000), (1, 8000)])
@pytest.mark.parametrize("N,C,F", [pytest.param(*g, id=f"{_route(g[0], g[1])}-{g[0]}x{g[1]}") for g in RATE_GEOMS])
def test_a_rate_between_two_table_rates_is_the_next_one(be, N, C, F, srate, snapped):
    q, tq = _ints(N, C, F, 16, snapped)
    got = check(be, q, tq, 16, srate, f"{N}x{C} {srate} Hz", "rates")
    assert got.tobytes() == be.p1_digital(q, tq, N, C, 16, snapped).tobytes(), f"{srate} Hz is not decoded as {snapped} Hz"


def _digital_into(be, q, tq, N, C, bits, srate, fill):
    """frad_p1_digital into a buffer of ``fill``: -> (the buffer afterwards, the FradError the call raised or None)"""
    from frad_python_amd._lib import FradError
    F, err = q.shape[0], None
    if be.name == "emu":
        out = np.full((F, N, C), fill)
        qq, tt = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(tq, np.int32)
        try:
            be.lib.p1_digital(qq.ctypes.data, tt.ctypes.data, F, N, C, bits, srate, out.ctypes.data)
        except FradError as e:
            err = e
        return out, err
    from frad_python_amd import _lib
    t = be.torch
    qq, tt = t.from_numpy(np.ascontiguousarray(q, np.int32)).to(be.dev), t.from_numpy(np.ascontiguousarray(tq, np.int32)).to(be.dev)
    out = t.full((F, N, C), fill, dtype=t.float64, device=be.dev)
    try:
        _lib.load().p1_digital(qq.data_ptr(), tt.data_ptr(), F, N, C, bits, srate, out.data_ptr(), int(t.cuda.current_stream().cuda_stream))
    except FradError as e:
        err = e
    t.cuda.synchronize()
    return out.cpu().numpy(), err


@pytest.mark.parametrize("N,C,F", [pytest.param(*g, id=f"{g[0]}x{g[1]}") for g in RATE_GEOMS])
def test_a_rate_above_the_table_is_refused_and_nothing_written(be, N, C, F):
    from frad_python_amd._lib import FradError
    q, tq = _ints(N, C, F)
    out, err = _digital_into(be, q, tq, N, C, 16, 96000, -7.0)
    assert err is None and np.all(out != -7.0)                 # the sentinel is no value a decode gives
    out, err = _digital_into(be, q, tq, N, C, 16, 96001, -7.0)
    assert isinstance(err, FradError) and err.status == -1     # FRAD_E_INVALID
    assert np.all(out == -7.0), "a refused call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------------
# 4. every legal compact size
# ---------------------------------------------------------------------------------------------------------------------
NEW_STEREO_SIZES = (160, 192, 224, 256, 320, 384, 448, 768, 1280, 3584)                    # no decode test had these


def _size_cases():
    out = [(f"{_route(N, 1)}-{N}x1", N, 1, 2) for N in sorted(fo.COMPACT_SAMPLES)]
    out += [(f"{_route(N, 2)}-{N}x2", N, 2, 2) for N in NEW_STEREO_SIZES]
    return out + [(f"{_route(4096, 6)}-4096x6", 4096, 6, 2)]


def _size_on_emu(N, C, F):
    """the emulator leg: every size up to 4096 and one workspace size; the channel groups run on the device only"""
    return (N <= 4096 or N == 10240) and C <= 2


def test_the_size_cases_reach_every_route():
    assert len(fo.COMPACT_SAMPLES) == 32
    gpu = {cid.split("-")[0] for cid, *_ in _size_cases()}
    emu = {cid.split("-")[0] for cid, *case in _size_cases() if _size_on_emu(*case)}
    assert gpu == {"wave", "inv256", "inv1024", "grp", "mixed", "direct", "workspace"}
    assert emu == {"wave", "inv256", "mixed", "direct", "workspace"}


@pytest.mark.parametrize("be,N,C,F", _legs(_size_cases(), _size_on_emu), indirect=["be"])
def test_every_compact_size(be, N, C, F):
    q, tq = _ints(N, C, F)
    check(be, q, tq, 16, 48000, f"{_route(N, C)} {N}x{C}", "every compact size")


@pytest.mark.parametrize("N,C,F", [pytest.param(128, 2, 7, id="inv256-128x2-7frames"), pytest.param(256, 1, 5, id="inv256-256x1-5frames")])
def test_frame_counts_that_do_not_fill_the_last_block(be, N, C, F):
    q, tq = _ints(N, C, F)
    check(be, q, tq, 16, 48000, f"{N}x{C}, {F} frames", "frames per block, band geometry")


# ---------------------------------------------------------------------------------------------------------------------
# 5. band geometry: empty bands (small frames at high rates) and band starts at or beyond N (low rates)
# ---------------------------------------------------------------------------------------------------------------------
def _codes_behind(tq, first, seed):
    """band codes first .. 26, which the encoder leaves 0 behind an empty band (p1tools.py:22), set to 1 .. 60"""
    tq = tq.copy()
    tq[:, first:] = np.random.default_rng(seed).integers(1, 61, tq[:, first:].shape)
    return tq


@pytest.mark.parametrize("srate", [96000, 88200])
@pytest.mark.parametrize("N,C,F", [pytest.param(128, 1, 3, id="inv256-128x1"), pytest.param(160, 2, 2, id="direct-160x2")])
def test_empty_bands(be, N, C, F, srate):
    """mapping_from_opus writes nothing for an empty band and carries on (p1tools.py:35-41): the codes behind it still shape the
    ramp of the band before them"""
    e = clipped_edges(N, srate)
    empty = [i for i in range(fo.N_BANDS - 1) if e[i + 1] <= e[i] < N]
    assert empty, "no empty band below N: the case tests nothing"
    q, tq = _ints(N, C, F, 16, srate)
    assert not tq[:, empty[0]:].any()                          # (the encoder side breaks at the empty band)
    tq = _codes_behind(tq, empty[0], N + srate)
    check(be, q, tq, 16, srate, f"{N}x{C} {srate} Hz, bands {empty} empty", "frames per block, band geometry")


@pytest.mark.parametrize("srate", [8000, 11025])
@pytest.mark.parametrize("N,C,F", [pytest.param(2048, 2, 2, id="wave-2048x2"), pytest.param(1024, 1, 2, id="inv256-1024x1")])
def test_band_starts_beyond_the_frame(be, N, C, F, srate):
    """band starts at or beyond N are clipped, bins behind the last start are 0; the first code behind N ends the last ramp"""
    raw = fo.band_edges(N, srate)
    beyond = [i for i in range(fo.N_BANDS) if raw[i] >= N]
    assert beyond, "no band starts at or beyond N: the case tests nothing"
    q, tq = _ints(N, C, F, 16, srate)
    tq = _codes_behind(tq, beyond[0], N + srate)
    if N == 2048:
        assert not marked(q, tq).any()
    check(be, q, tq, 16, srate, f"{N}x{C} {srate} Hz, bands {beyond[0]}.. start beyond N", "frames per block, band geometry")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the edges of the wave kernel's tables (|q| <= 255, codes 0 .. 255), zero frames
# ---------------------------------------------------------------------------------------------------------------------
def _table_edge_frames(C):
    q, tq = (a.copy() for a in _ints(2048, C, 3))
    assert not marked(q, tq).any()
    q[0, 5, 0] = 255; q[0, 700, C - 1] = -255; q[0, 2047, 0] = 255       # frame 0: the tables' last entries, nothing beyond
    tq[0, 3, 0] = 255; tq[0, 26, C - 1] = 255
    q[1, 9, C - 1] = 256                                                 # frame 1: the first |q| the table does not hold
    tq[2, 3, C - 1] = 256                                                # frame 2: the first code it does not hold
    if C == 1:
        q[2, 11, 0] = INT32_MIN; q[2, 1200, 0] = INT32_MAX               # what frad_p1_golomb_decode saturates to
    return q, tq


@pytest.mark.parametrize("C", [pytest.param(2, id="wave+redo-2048x2"), pytest.param(1, id="wave+redo-2048x1")])
def test_last_table_entries_and_the_first_values_beyond(be, C):
    N = 2048
    q, tq = _table_edge_frames(C)
    assert list(marked(q, tq)) == [False, True, True]
    got = check(be, q, tq, 16, 48000, f"{N}x{C} table edges", "table edges, zero frames")
    alone = check(be, q[:1], tq[:1], 16, 48000, f"{N}x{C} frame 0 alone", "table edges, zero frames")
    assert got[0].tobytes() == alone[0].tobytes(), "a marked neighbour changed an unmarked frame"


@pytest.mark.parametrize("C", [pytest.param(2, id="wave-2048x2"), pytest.param(1, id="wave-2048x1")])
def test_zero_frames(be, C):
    N = 2048
    q, tq = (a.copy() for a in _ints(N, C, 3))
    q[0] = 0; tq[0] = 0                                        # all zero
    tq[1] = 0                                                  # thresholds (e/2)^0 = 1 everywhere below the last band start
    assert not marked(q, tq).any() and q[1].any()
    got = check(be, q, tq, 16, 48000, f"{N}x{C} zero frames", "table edges, zero frames")
    assert not got[0].any() and not np.signbit(got[0]).any(), "an all-zero frame does not decode to +0.0"


# ---------------------------------------------------------------------------------------------------------------------
# 7. a batch is its frames alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,F", [pytest.param(2048, 1, 37, id="wave+redo-2048x1-37frames"), pytest.param(2048, 2, 23, id="wave+redo-2048x2-23frames"),
                                   pytest.param(640, 1, 9, id="mixed-640x1-9frames"), pytest.param(128, 1, 11, id="inv256-128x1-11frames")])
def test_batch_equals_its_frames_alone(be, N, C, F):
    q, tq = (a.copy() for a in _ints(N, C, F))
    if N == 2048:
        assert not marked(q, tq).any()
        q[5, 17, 0] = 1000; tq[F - 2, 3, C - 1] = 300          # two frames for the kernel behind the wave kernel
        assert list(np.flatnonzero(marked(q, tq))) == [5, F - 2]
    got = check(be, q, tq, 16, 48000, f"{N}x{C}, batch of {F}", "batches")
    for f in range(F):
        alone = be.p1_digital(q[f:f + 1], tq[f:f + 1], N, C, 16, 48000)
        assert alone[0].tobytes() == got[f].tobytes(), f"frame {f} alone differs from the batch"


# ---------------------------------------------------------------------------------------------------------------------
# 8. converted output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["s16le", "f32le", "s32be", "u8"])
@pytest.mark.parametrize("N,C", [pytest.param(2048, 2, id="wave-2048x2"), pytest.param(2048, 3, id="inv256-2048x3"), pytest.param(512, 2, id="inv256-512x2"),
                                 pytest.param(640, 1, id="mixed-640x1"), pytest.param(128, 2, id="inv256-128x2")])
def test_converted_output_is_from_f64_of_the_float64_output(be, N, C, fmt):
    q, tq = _ints(N, C, 2, 24)
    f64 = check(be, q, tq, 24, 48000, f"{N}x{C} bits 24", "depths")
    dt = fo.pcm_dtype(fmt)
    with np.errstate(all="ignore"):
        want = fo.from_f64(f64, dt).astype(dt)
    assert be.p1_digital_pcm(q, tq, N, C, 24, 48000, fmt).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 9. overlap-add (decoder.py:28-46, Hann ramp of backend/__init__.py:3)
# ---------------------------------------------------------------------------------------------------------------------
def ola_model(frames, ratio, prev_tail=None):
    """-> (out [F, cut, C], next_tail [N - cut, C]).  Frame i keeps rows [0, cut), its first L = N - cut rows faded in over the
    tail of frame i - 1 faded out: frame *= w, then frame += tail * w reversed -- two roundings each, in that order.  With
    ratio >= 2 L <= cut, so a frame's tail is never itself cross-faded."""
    F, N, C = frames.shape
    cut = N * (ratio - 1) // ratio
    L = N - cut
    assert 0 <= L <= cut
    w = 0.5 * (1 - np.cos(np.pi * np.arange(1, L + 1) / (L + 1)))
    out = frames[:, :cut].copy()
    for f in range(F):
        tail = frames[f - 1, cut:] if f else prev_tail
        if tail is not None and L:
            head = frames[f, :L] * w[:, None]
            out[f, :L] = head + tail * w[::-1, None]
    return out, frames[F - 1, cut:].copy()


def test_ola_model_is_the_oracles_overlap_add():
    rng = np.random.default_rng(1)
    for (N, C, ratio) in ((128, 2, 2), (160, 1, 3), (128, 1, 255), (640, 2, 256)):
        frames = rng.uniform(-1.1, 1.1, (4, N, C))
        ola = fo.OverlapAdd()
        want = np.stack([ola.push(f.copy(), True, ratio) for f in frames])
        out, tail = ola_model(frames, ratio)
        assert out.tobytes() == want.tobytes() and tail.tobytes() == ola.fragment.tobytes()


def _ola_check(be, frames, ratio, prev_tail, what):
    want, wtail = ola_model(frames, ratio, prev_tail)
    got, gtail = be.p1_ola(frames, ratio, prev_tail)
    assert got.shape == want.shape and gtail.shape == wtail.shape
    d = np.abs(got - want)
    print(f"[p1 decode] {be.name} overlap-add {what}: {np.count_nonzero(got != want)} of {got.size} values differ from the model, max {d.max():.3g}")
    assert got.tobytes() == want.tobytes(), f"{what}: the overlap-added frames are not the model's"
    assert gtail.tobytes() == wtail.tobytes(), f"{what}: the tail is not the last frame's"
    return got, gtail


@pytest.mark.parametrize("ratio", [2, 3, 16, 255, 256])
@pytest.mark.parametrize("N,C,F", [(640, 2, 4), (128, 1, 3)])
def test_overlap_add_at_every_kind_of_ratio(be, N, C, F, ratio):
    """ratios 255 and 256 leave L = 3 rows at N = 640 and a single row at N = 128 (cut = N (ratio - 1) // ratio)"""
    rng = np.random.default_rng(N + ratio)
    frames = rng.uniform(-1.1, 1.1, (F, N, C))
    L = N - N * (ratio - 1) // ratio
    assert L == {(640, 2): 320, (640, 3): 214, (640, 16): 40, (640, 255): 3, (640, 256): 3,
                 (128, 2): 64, (128, 3): 43, (128, 16): 8, (128, 255): 1, (128, 256): 1}[(N, ratio)]
    whole, tail = _ola_check(be, frames, ratio, None, f"{N}x{C} ratio {ratio}")
    prev = rng.uniform(-1.1, 1.1, (L, C))
    _ola_check(be, frames, ratio, prev, f"{N}x{C} ratio {ratio} with a tail")
    # two batches are one: the second continues from the first one's tail
    first, t1 = be.p1_ola(frames[:2], ratio)
    second, t2 = be.p1_ola(frames[2:], ratio, t1)
    assert np.concatenate([first, second]).tobytes() == whole.tobytes() and t2.tobytes() == tail.tobytes()
    # the converting store
    pcm, ptail = be.p1_ola_pcm(frames, ratio, "s16le", prev)
    want, wtail = ola_model(frames, ratio, prev)
    with np.errstate(all="ignore"):
        assert pcm.tobytes() == fo.from_f64(want, np.dtype("<i2")).astype("<i2").tobytes()
    assert ptail.tobytes() == wtail.tobytes()


def test_overlap_add_beyond_one_pass_of_the_grid(be):
    """k_p1_ola runs at most 4096 blocks of 256 and loops: 300 frames x 1920 rows x 2 channels = 1 152 000 elements make the
    second pass run; every element and the tail are compared, and a batch that continues from that tail"""
    F, N, C, ratio = 300, 2048, 2, 16
    rng = np.random.default_rng(300)
    frames = rng.uniform(-1.1, 1.1, (F + 2, N, C))
    assert F * (N * (ratio - 1) // ratio) * C == 1152000 > 4096 * 256
    got, tail = _ola_check(be, frames[:F], ratio, None, f"{F} frames")
    _ola_check(be, frames[F:], ratio, tail, "2 frames behind them")
    pcm, ptail = be.p1_ola_pcm(frames[:F], ratio, "s16le")
    with np.errstate(all="ignore"):
        assert pcm.tobytes() == fo.from_f64(got, np.dtype("<i2")).astype("<i2").tobytes()
    assert ptail.tobytes() == tail.tobytes()
