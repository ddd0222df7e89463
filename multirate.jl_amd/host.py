"""Host-side mirror of the reference operator interface over the C ABI (ctypes).

Reference interface mirrored (paths relative to /root/reference):
  FIRFilter(h, ratio) / FIRFilter(h, rate, Nphi)        src/Filters.jl:158-189
  filt(self, x) / filt(h, x, ratio) / filt(h, x, rate, Nphi)   src/Filters.jl:475-873
  filt!(buffer, self, x)  (here ``filt_``)               src/Filters.jl:450,489,536,598,693
  taps2pfb, outputlength, inputlength, nextphase, reset  src/Filters.jl:284,352,396,433,244

Signals are numpy arrays (host path, ``mrhip_filt_host``) or torch tensors on a ROCm device
(device path, ``mrhip_filt_device`` on torch's current stream).  Shape ``(n,)`` is one channel;
shape ``(nchannels, n)`` (C-contiguous: one channel per row == one channel per column of a Julia
Matrix) is a batch of independent streams sharing taps and phase state.

No arithmetic is done in Python and nothing here imports ``oracle/``: if ``libmultirate_hip.so``
is missing, or no gfx950 device is visible, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np

try:  # torch first: its bundled libamdhip64 must be the one HIP runtime of the process
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for pure-numpy use
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))

F32, F64, C64, C128 = 0, 1, 2, 3
STANDARD, DECIMATOR, INTERPOLATOR, RATIONAL, ARBITRARY, FARROW = 0, 1, 2, 3, 4, 5
KIND_NAMES = {STANDARD: "FIRStandard", DECIMATOR: "FIRDecimator", INTERPOLATOR: "FIRInterpolator",
              RATIONAL: "FIRRational", ARBITRARY: "FIRArbitrary", FARROW: "FIRFarrow"}
NUMERICS_STRICT, NUMERICS_FUSED = 0, 1

_NP2DT = {np.dtype(np.float32): F32, np.dtype(np.float64): F64,
          np.dtype(np.complex64): C64, np.dtype(np.complex128): C128}
_DT2NP = {v: k for k, v in _NP2DT.items()}


class _DeviceResident:
    """What a Python-side mirror (``FIRFilter._rates``, ``._chan_taps``, ``._chan_farrow``) holds after a device-resident update
    (``set_channel_rates_device`` and its siblings): the values were computed on the GPU and installed in stream order, so the host
    knows their shape and nothing else.  Queries ask the library; binding such a filter again is refused."""

    def __init__(self, shape):
        self.shape = tuple(shape)

    def __len__(self):
        return self.shape[0]


class MultirateHIPError(RuntimeError):
    """Raised where the reference raises Julia ``error(...)`` (and for HIP/runtime failures)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[mrhip status {code}] {msg}")
        self.code = code


class _State(C.Structure):
    _fields_ = [("kind", C.c_int32), ("tap_dtype", C.c_int32), ("sample_dtype", C.c_int32),
                ("output_dtype", C.c_int32), ("nchannels", C.c_int64), ("hLen", C.c_int64),
                ("interpolation", C.c_int64), ("decimation", C.c_int64), ("Nphi", C.c_int64),
                ("tapsPerPhi", C.c_int64), ("historyLen", C.c_int64), ("phiIdx", C.c_int64),
                ("inputDeficit", C.c_int64), ("xIdx", C.c_int64), ("rate", C.c_double),
                ("phiAccumulator", C.c_double), ("alpha", C.c_double), ("delta", C.c_double)]


class ChannelState(C.Structure):
    """mrhip_channel_state: one channel of a filter with per-channel rates (FIRFilter.per_channel_rates)"""
    _fields_ = [("rate", C.c_double), ("delta", C.c_double), ("phiAccumulator", C.c_double), ("alpha", C.c_double),
                ("phiIdx", C.c_int64), ("inputDeficit", C.c_int64), ("xIdx", C.c_int64), ("last_count", C.c_int64)]


# every symbol include/multirate_hip.h declares: (name, restype, argtypes)
_vp, _i64, _i, _d = C.c_void_p, C.c_int64, C.c_int, C.c_double
_pi64 = C.POINTER(C.c_int64)

# the sixteen constructors: (taps or pnfb, hLen, tap dtype) + the family's middle part + (sample dtype, nchannels, device, out); a
# ``_rates`` constructor takes a pointer to the rates where the others take the rate
_CREATE = {"rational": ([_i64, _i64], ("", "_bank", "_bank_ctaps")),
           "arbitrary": ([_d, _i64], ("", "_ctaps", "_bank", "_bank_ctaps", "_rates")),
           "farrow": ([_d, _i64, _i64], ("", "_bank", "_pnfb", "_rates", "_rates_pnfb", "_ctaps", "_bank_ctaps", "_pnfb_ctaps"))}


def _create_rows():
    for family, (middle, variants) in _CREATE.items():
        for v in variants:
            mid = [_vp] + middle[1:] if "_rates" in v else middle
            yield "mrhip_create_" + family + v, _i, [_vp, _i64, _i] + mid + [_i, _i64, _i, C.POINTER(_vp)]


ABI = [
    ("mrhip_abi_version", _i, []),
    ("mrhip_last_error", C.c_char_p, []),
    ("mrhip_device_count", _i, []),
    ("mrhip_taps2pfb", _i64, [_vp, _i64, _i, _i64, _vp]),
    ("mrhip_nextphase", _i64, [_i64, _i64, _i64]),
    ("mrhip_outputlength_ratio", _i64, [_i64, _i64, _i64, _i64]),
    ("mrhip_inputlength_ratio", _i64, [_i64, _i64, _i64, _i64]),
    ("mrhip_polyfit", _i, [_vp, _i64, _i64, _vp]),
    ("mrhip_output_dtype", _i, [_i, _i]),
    ("mrhip_kaiserlength", _i, [_d, _d, _d, _pi64, C.POINTER(C.c_double)]),
    ("mrhip_kaiser", _i, [_i64, _d, _vp]),
    ("mrhip_firprototype", _i64, [_i64, _vp, _i, _i, _vp]),
    ("mrhip_firdes", _i64, [_i64, _vp, _i, _i, _d, _d, _vp, _vp]),
    ("mrhip_firdes_kaiser", _i64, [_vp, _i, _d, _d, _i, _d, _vp]),
    *_create_rows(),
    ("mrhip_filt_device_rates", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_filt_device_rates_ragged", _i, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_filt_device_rates_lens_device", _i, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_filt_device_rates_chained", _i, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_get_channel_states", _i, [_vp, _vp]),
    ("mrhip_set_channel_states", _i, [_vp, _vp, _vp]),
    ("mrhip_set_channel_rates", _i, [_vp, _vp]),
    ("mrhip_set_channel_taps", _i, [_vp, _vp, _i64, _i]),
    ("mrhip_set_channel_taps_farrow", _i, [_vp, _vp, _i64, _i]),
    ("mrhip_set_channel_pnfb", _i, [_vp, _vp, _i64, _i64]),
    ("mrhip_set_channel_rates_device", _i, [_vp, _vp, _d, _d, _vp]),
    ("mrhip_set_channel_taps_device", _i, [_vp, _vp, _i64, _i, _vp]),
    ("mrhip_set_channel_pnfb_device", _i, [_vp, _vp, _i64, _i64, _vp]),
    ("mrhip_set_channel_ctaps", _i, [_vp, _vp, _i64, _i]),
    ("mrhip_set_channel_ctaps_device", _i, [_vp, _vp, _i64, _i, _vp]),
    ("mrhip_set_channel_ctaps_farrow", _i, [_vp, _vp, _i64, _i]),
    ("mrhip_set_channel_pnfb_ctaps", _i, [_vp, _vp, _i64, _i64]),
    ("mrhip_set_channel_pnfb_ctaps_device", _i, [_vp, _vp, _i64, _i64, _vp]),
    ("mrhip_set_channel_taps_farrow_device", _i, [_vp, _vp, _i64, _i, _vp]),
    ("mrhip_set_channel_ctaps_farrow_device", _i, [_vp, _vp, _i64, _i, _vp]),
    ("mrhip_get_pnfb", _i, [_vp, _vp]),
    ("mrhip_farrow_tapsforphase", _i, [_vp, _d, _vp]),
    ("mrhip_arbitrary_tapsforphase", _i, [_vp, _d, _vp]),
    ("mrhip_destroy", None, [_vp]),
    ("mrhip_outputlength", _i64, [_vp, _i64]),
    ("mrhip_next_output_count", _i64, [_vp, _i64]),
    ("mrhip_advance_state", _i64, [_vp, _i64]),
    ("mrhip_inputlength", _i64, [_vp, _i64]),
    ("mrhip_get_state", _i, [_vp, C.POINTER(_State)]),
    ("mrhip_set_state", _i, [_vp, _i64, _i64, _d]),
    ("mrhip_get_history", _i, [_vp, _vp]),
    ("mrhip_set_history", _i, [_vp, _vp]),
    ("mrhip_reset", _i, [_vp]),
    ("mrhip_set_numerics", _i, [_vp, _i]),
    ("mrhip_set_mod_form", _i, [_vp, _i]),
    ("mrhip_get_taps", _i, [_vp, _i, _vp]),
    ("mrhip_filt_device", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _pi64, _vp]),
    ("mrhip_filt_device_async", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_filt_device_chained", _i, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_filt_device_multi", _i, [C.POINTER(_vp), _i, C.POINTER(_vp), _pi64, C.POINTER(_vp), _pi64, _pi64, _vp]),
    ("mrhip_outputlength_bound", _i64, [_vp, _i64]),
    ("mrhip_sync_state", _i, [_vp, _pi64]),
    ("mrhip_set_history_device", _i, [_vp, _vp, _vp]),
    ("mrhip_filt_device_chunked", _i, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _pi64, _vp]),
    ("mrhip_filt_host", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _pi64]),
    ("mrhip_synchronize", _i, [_vp, _vp]),
    ("mrhip_cascade_create", _i, [C.POINTER(_vp), _i, C.POINTER(_vp)]),
    ("mrhip_cascade_destroy", None, [_vp]),
    ("mrhip_cascade_outputlength", _i64, [_vp, _i64]),
    ("mrhip_cascade_next_output_count", _i64, [_vp, _i64]),
    ("mrhip_cascade_filt_device", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _pi64, _vp]),
    ("mrhip_cascade_filt_device_async", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    ("mrhip_cascade_reset", _i, [_vp]),
    ("mrhip_filt_once", _i, [_vp, _i64, _i, _i64, _i64, _d, _i64, _vp, _i64, _i, _vp, _i64, _pi64, _i]),
    ("mrhip_set_timing", _i, [_vp, _i]),
    ("mrhip_timing_read", _i, [_vp, _pi64, C.POINTER(C.c_double)]),
    ("mrhip_last_kernel_name", C.c_char_p, [_vp]),
    ("mrhip_schedule_info", _i, [_vp, _pi64, _i]),
    ("mrhip_sharded_create", _i, [_i, _vp, _i64, _i, _i64, _i64, _d, _i64, _i64, _i, _i64, C.POINTER(_i), _i, C.POINTER(_vp)]),
    ("mrhip_sharded_destroy", None, [_vp]),
    ("mrhip_sharded_nshards", _i, [_vp]),
    ("mrhip_sharded_shard", _i, [_vp, _i, _pi64, _pi64, C.POINTER(_i), C.POINTER(_vp)]),
    ("mrhip_sharded_outputlength", _i64, [_vp, _i64]),
    ("mrhip_sharded_next_output_count", _i64, [_vp, _i64]),
    ("mrhip_sharded_reset", _i, [_vp]),
    ("mrhip_sharded_filt_device", _i, [_vp, C.POINTER(_vp), _i64, _pi64, C.POINTER(_vp), _i64, _pi64, _pi64]),
    ("mrhip_sharded_filt_host", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _pi64]),
    ("mrhip_sharded_gather", _i, [_vp, C.POINTER(_vp), _i64, _pi64, _vp, _i64, _i]),
    ("mrhip_sharded_wait_stream", _i, [_vp, _i, _vp]),
    ("mrhip_sharded_signal_stream", _i, [_vp, _i, _vp]),
    ("mrhip_sharded_synchronize", _i, [_vp]),
    ("mrhip_ring_open", _i, [_vp, C.POINTER(_vp)]),
    ("mrhip_ring_push", _i, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _pi64, C.POINTER(C.c_uint64)]),
    ("mrhip_ring_push_chunks", _i, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _pi64, C.POINTER(C.c_uint64)]),
    ("mrhip_ring_wait", _i, [_vp, C.c_uint64]),
    ("mrhip_ring_drain", _i, [_vp]),
    ("mrhip_ring_close", _i, [_vp]),
    ("mrhip_ring_info", _i, [_vp, _pi64, _i]),
]

_lib = None


def library_path() -> str:
    # MRHIP_LIB_PATH: developer override used to A/B-test alternative builds of the same ABI
    return os.environ.get("MRHIP_LIB_PATH") or os.path.join(_HERE, "libmultirate_hip.so")


def load_library():
    """dlopen libmultirate_hip.so and bind every ABI symbol.  Raises if the library is missing --
    there is no fallback implementation."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise MultirateHIPError(-1, f"{path} not found: build it with `make -C multirate.jl_amd/csrc` "
                                        "(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(path)
        for name, res, args in ABI:
            fn = getattr(lib, name)  # AttributeError if the header and the .so ever disagree
            fn.restype = res
            fn.argtypes = args
        if lib.mrhip_abi_version() != 1:
            raise MultirateHIPError(-1, "ABI version mismatch")
        _lib = lib
    return _lib


def _check(rc: int):
    if rc != 0:
        raise MultirateHIPError(rc, load_library().mrhip_last_error().decode("utf-8", "replace"))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _as_taps(h, allow_complex: bool = False) -> np.ndarray:
    h = np.ascontiguousarray(h)
    if h.dtype == np.float32 or h.dtype == np.float64:
        return h
    if np.issubdtype(h.dtype, np.integer) or h.dtype == np.float16:
        return h.astype(np.float64)
    if h.dtype == np.complex64 or h.dtype == np.complex128:
        if allow_complex:
            return h
        raise MultirateHIPError(5, f"tap dtype {h.dtype}: complex taps are built with FIRFilter.complex_taps(h, ratio) "
                                   "(the rational family only); this constructor takes Float32/Float64 taps")
    raise MultirateHIPError(5, f"unsupported tap dtype {h.dtype} (taps must be Float32/Float64, or Complex64/Complex128 "
                               "through FIRFilter.complex_taps)")


# ---- the argument checks the FIRFilter classmethods share: `who` is the method, `other` what its message points to -----------------
def _takes_ratio(ratio, who: str, other: str):
    if isinstance(ratio, (float, np.floating)):
        raise MultirateHIPError(5, f"{who} builds the rational family only ({other})")


def _takes_rate(rate, who: str, other: str):
    if not isinstance(rate, (float, np.floating)):
        raise MultirateHIPError(1, f"{who} takes a floating-point rate (a Rational ratio: FIRFilter.{other})")


def _takes_polyorder(polyorder, who: str, other: str):
    if polyorder is None:
        raise MultirateHIPError(1, f"{who} takes a polyorder (without one: FIRFilter.{other})")


def _real_taps(h, who: str, other: str) -> np.ndarray:
    h = np.asarray(h)
    if h.dtype.kind == "c":
        raise MultirateHIPError(5, f"{who} takes Float32/Float64 taps ({other})")
    return h


def _complex_taps(h, who: str = "", other=None) -> np.ndarray:
    """complex taps as they are; real ones are promoted, or refused where the method has a sibling for them (`other`)"""
    h = np.ascontiguousarray(h)
    if h.dtype != np.complex64 and h.dtype != np.complex128:
        if other is not None:
            raise MultirateHIPError(1, f"{who} takes Complex64/Complex128 taps, got {h.dtype} (real taps: FIRFilter.{other})")
        h = h.astype(np.complex64 if h.dtype == np.float32 else np.complex128)
    return h


def _tap_matrix(H, who: str) -> np.ndarray:
    H = np.asarray(H)
    if H.ndim != 2 or H.shape[0] < 1 or H.shape[1] < 1:
        raise MultirateHIPError(1, f"{who} takes a (nchannels, hLen) matrix of taps; got shape {H.shape}")
    return H


def _pnfb_shape(f):
    if f._pnfb_in is not None and f._pnfb_in.shape != (f.tapsPerPhi, f.polyorder + 1):
        raise MultirateHIPError(1, f"pnfb must have shape (tapsPerPhi, polyorder+1) = {(f.tapsPerPhi, f.polyorder + 1)}")
    return f


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _torch_np_dtype(t):
    return {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64),
            torch.complex64: np.dtype(np.complex64), torch.complex128: np.dtype(np.complex128)}[t]


def _np_torch_dtype(d):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}[np.dtype(d)]


# ---- host-only helpers ------------------------------------------------------------------------
def taps2pfb(h, Nphi: int) -> np.ndarray:
    """taps2pfb(h, N𝜙), src/Filters.jl:284-298.  Returns the tapsPer𝜙 x N𝜙 matrix (complex for complex h)."""
    h = _as_taps(h, allow_complex=True)
    lib = load_library()
    T = lib.mrhip_taps2pfb(_ptr(h), len(h), _NP2DT[h.dtype], Nphi, None)
    if T < 0:
        raise MultirateHIPError(1, "bad taps2pfb arguments")
    out = np.empty(T * Nphi, dtype=h.dtype)
    lib.mrhip_taps2pfb(_ptr(h), len(h), _NP2DT[h.dtype], Nphi, _ptr(out))
    return out.reshape(Nphi, T).T.copy()


def polyfit(y, polyorder: int) -> np.ndarray:
    """polyfit(y, polyorder), src/support.jl:85-88: coefficients in ascending powers (Poly.a)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    out = np.zeros(polyorder + 1, dtype=np.float64)
    _check(load_library().mrhip_polyfit(_ptr(y), len(y), polyorder, _ptr(out)))
    return out


def nextphase(currentphase: int, ratio) -> int:
    """nextphase(currentphase, ratio), src/Filters.jl:433-439."""
    r = Fraction(ratio)
    return load_library().mrhip_nextphase(currentphase, r.numerator, r.denominator)


# ---- the filter object ------------------------------------------------------------------------
class FIRFilter:
    """FIRFilter(h, ratio::Rational = 1//1)  or  FIRFilter(h, rate::Float, N𝜙 = 32)
    or  FIRFilter(h, rate::Float, N𝜙, polyorder)  (FIRFarrow, src/Filters.jl:192-198).

    Mirrors src/Filters.jl:158-189: a ``Fraction``/int/(num, den) ratio selects FIRStandard,
    FIRDecimator, FIRInterpolator or FIRRational exactly as the reference does; a ``float`` selects
    FIRArbitrary.  Like the reference, whose ``history`` vector takes the sample type of the first
    ``filt`` call (src/Filters.jl:452), the device-side object is created on the first call, when
    the sample dtype and the number of channels are known.
    """

    def __init__(self, h, ratio=Fraction(1, 1), Nphi: int = 32, polyorder=None, *, device: int = 0,
                 numerics: int = NUMERICS_STRICT, pnfb=None, _complex_taps: bool = False):
        self._lib = load_library()
        self.h = _as_taps(h, allow_complex=_complex_taps).copy()
        if len(self.h) < 1:
            raise MultirateHIPError(1, "h must hold at least one tap")
        self.device = int(device)
        self.numerics = int(numerics)
        self._handle = None
        self._tx = None
        self._nch = None
        self.polyorder = None
        self._pnfb_in = None
        self._rates = None                # per-channel rates (FIRFilter.per_channel_rates, .per_channel_rates_farrow): Float64, one per channel; self.rate is the largest
        self._chan_taps = None            # per-channel taps ON TOP of per-channel rates (FIRFilter.set_channel_taps, .per_channel_taps_and_rates): the (nchannels, hLen) matrix, installed by mrhip_set_channel_taps
        self._chan_ctaps = None           # COMPLEX per-channel taps on top of per-channel rates (FIRFilter.set_channel_ctaps, .set_channel_ctaps_device, .per_channel_complex_taps_and_rates): the (nchannels, hLen) complex matrix, installed by mrhip_set_channel_ctaps; self.h stays the real placeholder the filter is created over
        self._farrow_ctaps = False        # the FIRFarrow mirror below holds COMPLEX banks (FIRFilter.set_channel_ctaps_farrow, .set_channel_pnfb_ctaps, .set_channel_pnfb_ctaps_device, .per_channel_complex_taps_and_rates_farrow): _chan_farrow is then ("ctaps", the complex (nchannels, hLen) matrix) or ("cpnfb", the complex banks); self.h stays the real vector the filter is created over
        self._chan_farrow = None          # the same for FIRFarrow (FIRFilter.set_channel_taps_farrow, .set_channel_pnfb, .per_channel_taps_and_rates_farrow): ("taps", the (nchannels, hLen) matrix) or ("pnfb", the (nchannels, tapsPer𝜙, polyorder+1) banks), whichever call came last
        self._bank = None                 # per-channel taps (FIRFilter.per_channel, .per_channel_complex_taps, .per_channel_arbitrary, .per_channel_complex_taps_arbitrary, .per_channel_farrow, .per_channel_complex_taps_farrow): the (nchannels, hLen) matrix; self.h is its row 0
        if isinstance(ratio, (float, np.floating)):
            if not ratio > 0.0:
                raise MultirateHIPError(1, "rate must be greater than 0")  # Filters.jl:184
            self.rate = float(ratio)
            self.ratio = None
            self.Nphi = int(Nphi)
            self.kind = ARBITRARY if polyorder is None else FARROW
            self.polyorder = None if polyorder is None else int(polyorder)
            # optional caller-fitted polynomial bank (tapsPerPhi x (polyorder+1), ascending powers)
            # (complex taps, FIRFilter.complex_taps_farrow: complex coefficients, handed over as (re, im) pairs of Float64)
            self._pnfb_in = None if pnfb is None else np.ascontiguousarray(pnfb, dtype=np.complex128 if self.h.dtype.kind == "c" else np.float64)
            self.interpolation, self.decimation = self.Nphi, 1
            self.tapsPerPhi = -(-len(self.h) // self.Nphi)
            self.historyLen = self.tapsPerPhi - 1
        else:
            if isinstance(ratio, tuple):
                ratio = Fraction(*ratio)
            self.ratio = Fraction(ratio)
            if self.ratio <= 0:
                raise MultirateHIPError(1, "ratio must be positive")
            self.rate = None
            L, M = self.ratio.numerator, self.ratio.denominator
            self.interpolation, self.decimation = L, M
            if L == 1 and M == 1:
                self.kind = STANDARD
            elif L == 1:
                self.kind = DECIMATOR
            elif M == 1:
                self.kind = INTERPOLATOR
            else:
                self.kind = RATIONAL
            self.Nphi = L
            self.tapsPerPhi = len(self.h) if L == 1 else -(-len(self.h) // L)
            self.historyLen = self.tapsPerPhi - 1

    @classmethod
    def complex_taps(cls, h, ratio=1, *, device: int = 0):
        """FIRFilter(h::Vector{Complex64 / Complex128}, ratio::Rational): the reference is generic over the tap type
        (src/Filters.jl:158-180, src/support.jl:5-55), so a rotated low-pass, a Hilbert or a single-sideband filter in
        front of a resampler is just a FIRFilter there.  Rational family only (FIRStandard, FIRDecimator, FIRInterpolator,
        FIRRational); the output is always complex (Complex128 if either side is 64-bit).  Real ``h`` is promoted to
        complex.  STRICT numerics only (include/multirate_hip.h: complex taps)."""
        _takes_ratio(ratio, "complex_taps", "a float rate: FIRFilter.complex_taps_arbitrary; FIRFarrow takes Float32/Float64 taps")
        return cls(_complex_taps(h), ratio, device=device, _complex_taps=True)

    @classmethod
    def complex_taps_arbitrary(cls, h, rate, Nphi: int = 32, *, device: int = 0):
        """FIRFilter(h::Vector{Complex64 / Complex128}, rate::Float, N𝜙 = 32): FIRArbitrary with complex taps
        (FIRArbitrary(h, rate, N𝜙), src/Filters.jl:105-117, is generic over the tap type: dh = [diff(h), 0], both filter banks
        and tapsforphase are complex).  The output is always complex (Complex128 if either side is 64-bit); real ``h`` is
        promoted to complex.  STRICT numerics only (include/multirate_hip.h: complex taps).  The device object is created by
        ``mrhip_create_arbitrary_ctaps``."""
        _takes_rate(rate, "complex_taps_arbitrary", "complex_taps")
        return cls(_complex_taps(h), float(rate), int(Nphi), device=device, _complex_taps=True)

    @classmethod
    def complex_taps_farrow(cls, h, rate, Nphi, polyorder, *, pnfb=None, device: int = 0):
        """FIRFilter(h::Vector{Complex64 / Complex128}, rate::Float, N𝜙, polyorder): FIRFarrow with complex taps
        (FIRFarrow(h, rate, N𝜙, polyorder), src/Filters.jl:138-147, is generic over the tap type: one Poly{Complex{T}} per row of
        the filter bank, fitted per component; tapsforphase and pnfb() are complex).  ``pnfb``: a caller-fitted bank, complex, shape
        (tapsPer𝜙, polyorder+1), ascending powers.  The output is always complex (Complex128 if either side is 64-bit); real
        ``h`` is promoted to complex.  STRICT numerics only (include/multirate_hip.h: complex taps).  The device object is created
        by ``mrhip_create_farrow_ctaps`` / ``mrhip_create_farrow_pnfb_ctaps``."""
        _takes_rate(rate, "complex_taps_farrow", "complex_taps")
        _takes_polyorder(polyorder, "complex_taps_farrow", "complex_taps_arbitrary")
        return _pnfb_shape(cls(_complex_taps(h), float(rate), int(Nphi), int(polyorder), device=device, pnfb=pnfb, _complex_taps=True))

    @classmethod
    def per_channel(cls, H, ratio=1, *, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(H[c], ratio) per channel behind one filter object: in the reference N channels are N FIRFilter objects and
        every ``h`` may differ (per-antenna equalisers, matched-filter banks, calibration filters in front of a common resampler).
        ``H``: shape (nchannels, hLen), Float32 or Float64.  Ratio, state and call length are shared, only the taps differ; channel
        c is bit for bit ``FIRFilter(H[c], ratio)`` fed ``x[c]`` (include/multirate_hip.h: per-channel taps).  Rational family
        only.  The filter binds to exactly ``H.shape[0]`` channels; ``taps()`` has shape (nchannels, tapsPer𝜙, N𝜙).  The device
        object is created by ``mrhip_create_rational_bank``."""
        _takes_ratio(ratio, "per_channel", "a float rate: FIRFilter.per_channel_arbitrary, FIRFilter.per_channel_farrow")
        H = _tap_matrix(_real_taps(H, "per_channel", "complex taps in a bank are not supported"), "per_channel")
        return cls._of_bank(_as_taps(H), ratio, device=device, numerics=numerics)

    @classmethod
    def per_channel_complex_taps(cls, H, ratio=1, *, device: int = 0):
        """One FIRFilter(H[c]::Vector{Complex64 / Complex128}, ratio) per channel behind one filter object: one low-pass prototype
        rotated to every channel's own centre frequency in front of a common resampler, per-channel Hilbert or single-sideband
        filters, per-antenna complex equalisers.  ``H``: shape (nchannels, hLen); real ``H`` is promoted to complex, as
        ``complex_taps`` does.  Channel c is bit for bit ``FIRFilter.complex_taps(H[c], ratio)`` fed ``x[c]``
        (include/multirate_hip.h: per-channel complex taps).  Rational family only; the output is always complex (Complex128 if
        either side is 64-bit); STRICT numerics only.  The filter binds to exactly ``H.shape[0]`` channels; ``taps()`` has shape
        (nchannels, tapsPer𝜙, N𝜙), complex.  The device object is created by ``mrhip_create_rational_bank_ctaps``."""
        _takes_ratio(ratio, "per_channel_complex_taps", "a float rate: FIRFilter.per_channel_complex_taps_arbitrary, FIRFilter.per_channel_complex_taps_farrow")
        return cls._of_bank(_complex_taps(_tap_matrix(H, "per_channel_complex_taps")), ratio, device=device, _complex_taps=True)

    @classmethod
    def per_channel_arbitrary(cls, H, rate, Nphi: int = 32, *, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(H[c], rate::Float, N𝜙) per channel behind one filter object: FIRArbitrary with per-channel taps (per-antenna
        equalisers folded into the prototype of a clock-trim resampler, per-channel matched pulse shapes in front of a common
        symbol-rate change, per-sensor calibration filters).  ``H``: shape (nchannels, hLen), Float32 or Float64.  The phase schedule
        does not depend on the taps: rate, N𝜙, state and call length are shared, only the two filter banks differ; channel c is bit
        for bit ``FIRFilter(H[c], rate, Nphi)`` fed ``x[c]``, under STRICT and FUSED (include/multirate_hip.h: per-channel taps for
        FIRArbitrary).  The filter binds to exactly ``H.shape[0]`` channels; ``taps(which)`` has shape (nchannels, tapsPer𝜙, N𝜙) and
        ``tapsforphase`` (nchannels, tapsPer𝜙).  The device object is created by ``mrhip_create_arbitrary_bank``."""
        _takes_rate(rate, "per_channel_arbitrary", "per_channel")
        H = _tap_matrix(_real_taps(H, "per_channel_arbitrary", "complex taps: FIRFilter.per_channel_complex_taps_arbitrary"), "per_channel_arbitrary")
        return cls._of_bank(_as_taps(H), float(rate), int(Nphi), device=device, numerics=numerics)

    @classmethod
    def per_channel_rates(cls, h, rates, Nphi: int = 32, *, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(h, rates[c]::Float, N𝜙) per channel behind one filter object: FIRArbitrary with per-channel RATES (receivers
        each off its own clock trimmed to a common rate, per-emitter Doppler time-scale correction, per-channel fractional delay).
        ``h``: one Float32 or Float64 tap vector, shared; ``rates``: one rate > 0 per channel.  Every channel has its own phase
        schedule, state and output count; channel c is bit for bit ``FIRFilter(h, rates[c], Nphi)`` fed ``x[c]``, under STRICT and
        FUSED (include/multirate_hip.h: per-channel rates for FIRArbitrary).  The filter binds to exactly ``len(rates)`` channels and
        takes device tensors: ``filt(x)`` returns a list of ``nchannels`` arrays, ``filt_into(buffer, x)`` the int64 counts,
        ``channel_states`` / ``set_channel_states`` replace ``state`` / ``set_state``.  What carries one state or one count
        (``state``, ``outputlength``, ``next_output_count``, ``filt_into_async``, rings, cascades, ...) raises status 5.  The device
        object is created by ``mrhip_create_arbitrary_rates``."""
        h = _real_taps(h, "per_channel_rates", "complex taps with per-channel rates are left out")
        r = cls._checked_rates(rates, "per_channel_rates")
        f = cls(h, float(r.max()), int(Nphi), device=device, numerics=numerics)
        f._rates = r
        return f

    @classmethod
    def per_channel_taps_and_rates(cls, H, rates, Nphi: int = 32, *, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(H[c], rates[c]::Float, N𝜙) per channel behind one filter object: FIRArbitrary with per-channel taps AND
        per-channel rates (receivers each off its own clock, each with its own front-end equaliser or calibration filter; per-emitter
        Doppler correction with the emitter's own matched pulse).  ``H``: shape (nchannels, hLen), Float32 or Float64; ``rates``: one
        rate > 0 per channel.  It is the filter of ``per_channel_rates(H[0], rates, Nphi)`` followed by ``set_channel_taps(H)``:
        channel c is bit for bit ``FIRFilter(H[c], rates[c], Nphi)`` fed ``x[c]``, under STRICT and FUSED (include/multirate_hip.h:
        per-channel taps with per-channel rates for FIRArbitrary).  ``taps(which)`` has shape (nchannels, tapsPer𝜙, N𝜙) and
        ``tapsforphase`` (nchannels, tapsPer𝜙); everything else behaves as on the filter of ``per_channel_rates``."""
        who = "per_channel_taps_and_rates"
        H = _as_taps(_tap_matrix(_real_taps(H, who, "complex taps with per-channel rates are left out"), who))
        f = cls.per_channel_rates(H[0], rates, Nphi, device=device, numerics=numerics)
        f.set_channel_taps(H)
        return f

    @classmethod
    def per_channel_complex_taps_and_rates(cls, H, rates, Nphi: int = 32, *, device: int = 0):
        """One FIRFilter(H[c]::Vector{Complex}, rates[c]::Float, N𝜙) per channel behind one filter object: FIRArbitrary with COMPLEX
        per-channel taps and per-channel rates (per-emitter Doppler correction: a time scale and a carrier offset per channel).
        ``H``: shape (nchannels, hLen), complex64 or complex128; ``rates``: one rate > 0 per channel.  It is the two steps in one:
        the filter of ``per_channel_rates`` over placeholder taps ``real(H[0])`` of the same length and precision, followed by
        ``set_channel_ctaps(H)``.  Channel c is bit for bit ``FIRFilter.complex_taps_arbitrary(H[c], rates[c], Nphi)`` fed ``x[c]``
        (include/multirate_hip.h: complex per-channel taps with per-channel rates for FIRArbitrary).  STRICT only."""
        who = "per_channel_complex_taps_and_rates"
        H = np.asarray(H)
        if H.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise MultirateHIPError(1, f"{who} takes complex64 or complex128 taps; real taps: FIRFilter.per_channel_taps_and_rates")
        H = _tap_matrix(H, who)
        f = cls.per_channel_rates(np.ascontiguousarray(H[0].real), rates, Nphi, device=device)
        f.set_channel_ctaps(H)
        return f

    @staticmethod
    def _checked_rates(rates, who):
        """one finite rate > 0 per channel, at least one, as a Float64 vector (the checks the library repeats)"""
        r = np.atleast_1d(np.asarray(rates, dtype=np.float64))
        if r.ndim != 1 or r.size < 1:
            raise MultirateHIPError(1, f"{who} takes one rate per channel, at least one; got shape {r.shape}")
        if not np.all(np.isfinite(r)) or not np.all(r > 0.0):
            raise MultirateHIPError(1, "rate must be greater than 0 (every channel's)")      # Filters.jl:184
        return np.ascontiguousarray(r).copy()

    @classmethod
    def per_channel_rates_farrow(cls, h, rates, Nphi: int = 32, polyorder=4, *, pnfb=None, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(h, rates[c]::Float, N𝜙, polyorder) per channel behind one filter object: FIRFarrow with per-channel RATES
        (the same users as ``per_channel_rates``; FIRFarrow is the reference's kernel for a continuously variable rate).  ``h``: one
        Float32 or Float64 tap vector, shared -- so ONE polynomial bank, fitted once, or ``pnfb``: a caller-fitted bank of shape
        (tapsPer𝜙, polyorder+1), ascending powers; ``rates``: one rate > 0 per channel.  Every channel has its own phase schedule,
        state and output count; channel c is bit for bit ``FIRFilter(h, rates[c], Nphi, polyorder)`` fed ``x[c]``, under STRICT and
        FUSED (include/multirate_hip.h: per-channel rates for FIRFarrow).  ``filt``, ``filt_into``, ``channel_states``,
        ``set_channel_states``, ``set_channel_rates``, ``outputlength_bound``, ``reset`` and ``history`` behave as on the filter of
        ``per_channel_rates``; ``pnfb()`` and ``tapsforphase`` as on a one-channel FIRFarrow filter.  The device object is created by
        ``mrhip_create_farrow_rates`` / ``mrhip_create_farrow_rates_pnfb``."""
        h = _real_taps(h, "per_channel_rates_farrow", "complex taps with per-channel rates are left out")
        _takes_polyorder(polyorder, "per_channel_rates_farrow", "per_channel_rates")
        r = cls._checked_rates(rates, "per_channel_rates_farrow")
        if not 0 <= int(polyorder) <= 32 or (pnfb is None and int(polyorder) + 1 > int(Nphi)):
            raise MultirateHIPError(1, "polyorder must be in 0..min(32, Nphi-1)")
        f = _pnfb_shape(cls(h, float(r.max()), int(Nphi), int(polyorder), device=device, numerics=numerics, pnfb=pnfb))
        f._rates = r
        return f

    @classmethod
    def per_channel_taps_and_rates_farrow(cls, H, rates, Nphi: int = 32, polyorder=4, *, pnfb=None, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(H[c], rates[c]::Float, N𝜙, polyorder) per channel behind one filter object: FIRFarrow with per-channel taps AND
        per-channel rates (Doppler and clock trackers that call ``set_channel_rates`` every chunk and carry a per-emitter matched pulse
        or a per-receiver equaliser).  ``H``: shape (nchannels, hLen), Float32 or Float64; ``rates``: one rate > 0 per channel.  It is
        the filter of ``per_channel_rates_farrow(H[0], rates, Nphi, polyorder)`` followed by ``set_channel_taps_farrow(H)`` -- every row
        fitted on its own -- or, with ``pnfb`` of shape (nchannels, tapsPer𝜙, polyorder+1), by ``set_channel_pnfb(pnfb)``: caller-fitted
        banks in ascending powers, ``H`` then only gives hLen and the tap dtype.  Channel c is bit for bit
        ``FIRFilter(H[c], rates[c], Nphi, polyorder)`` (on bank c) fed ``x[c]``, under STRICT and FUSED (include/multirate_hip.h:
        per-channel taps with per-channel rates for FIRFarrow).  ``pnfb()`` has shape (nchannels, tapsPer𝜙, polyorder+1) and
        ``tapsforphase`` (nchannels, tapsPer𝜙); everything else behaves as on the filter of ``per_channel_rates_farrow``."""
        who = "per_channel_taps_and_rates_farrow"
        H = _as_taps(_tap_matrix(_real_taps(H, who, "complex taps with per-channel rates are left out"), who))
        if pnfb is None:
            f = cls.per_channel_rates_farrow(H[0], rates, Nphi, polyorder, device=device, numerics=numerics)
            f.set_channel_taps_farrow(H)
        else:
            PN = np.asarray(pnfb)
            if PN.ndim != 3 or PN.shape[0] < 1:
                raise MultirateHIPError(1, f"{who} takes pnfb of shape (nchannels, tapsPerPhi, polyorder+1); got {PN.shape}")
            f = cls.per_channel_rates_farrow(H[0], rates, Nphi, polyorder, pnfb=PN[0], device=device, numerics=numerics)
            f.set_channel_pnfb(PN)
        return f

    @classmethod
    def per_channel_complex_taps_and_rates_farrow(cls, H, rates, Nphi: int = 32, polyorder=4, *, pnfb=None, device: int = 0):
        """One FIRFilter(H[c]::Vector{Complex}, rates[c]::Float, N𝜙, polyorder) per channel behind one filter object: FIRFarrow with
        COMPLEX per-channel taps and per-channel rates (per-emitter Doppler correction with a tracker that calls ``set_channel_rates``
        every chunk: a time scale and a carrier offset per channel).  ``H``: shape (nchannels, hLen), complex64 or complex128;
        ``rates``: one rate > 0 per channel.  It is the two steps in one: the filter of ``per_channel_rates_farrow`` over placeholder
        taps ``real(H[0])`` of the same length and precision, followed by ``set_channel_ctaps_farrow(H)`` -- every row fitted on its
        own -- or, with a complex ``pnfb`` of shape (nchannels, tapsPer𝜙, polyorder+1), by ``set_channel_pnfb_ctaps(pnfb)``: ``H`` then
        only gives hLen and the precision.  Channel c is bit for bit ``FIRFilter.complex_taps_farrow(H[c], rates[c], Nphi, polyorder)``
        (on bank c) fed ``x[c]`` (include/multirate_hip.h: complex per-channel taps with per-channel rates for FIRFarrow).  STRICT
        only."""
        who = "per_channel_complex_taps_and_rates_farrow"
        H = np.asarray(H)
        if H.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise MultirateHIPError(1, f"{who} takes complex64 or complex128 taps; real taps: FIRFilter.per_channel_taps_and_rates_farrow")
        H = _tap_matrix(H, who)
        if pnfb is None:
            f = cls.per_channel_rates_farrow(np.ascontiguousarray(H[0].real), rates, Nphi, polyorder, device=device)
            f.set_channel_ctaps_farrow(H)
        else:
            PN = np.asarray(pnfb)
            if PN.ndim != 3 or PN.shape[0] < 1 or PN.dtype.kind != "c":
                raise MultirateHIPError(1, f"{who} takes a complex pnfb of shape (nchannels, tapsPerPhi, polyorder+1); got {PN.dtype} {PN.shape}")
            f = cls.per_channel_rates_farrow(np.ascontiguousarray(H[0].real), rates, Nphi, polyorder, pnfb=np.ascontiguousarray(PN[0].real), device=device)
            f.set_channel_pnfb_ctaps(PN)
        return f

    @classmethod
    def per_channel_complex_taps_arbitrary(cls, H, rate, Nphi: int = 32, *, device: int = 0):
        """One FIRFilter(H[c]::Vector{Complex64 / Complex128}, rate::Float, N𝜙) per channel behind one filter object: FIRArbitrary
        with per-channel complex taps (a prototype rotated to every channel's own centre frequency in front of a common clock-trim or
        arbitrary-rate change, per-antenna complex equalisers folded into the resampler's prototype, per-channel Hilbert or
        single-sideband filters in front of a symbol-rate change).  ``H``: shape (nchannels, hLen), Complex64 or Complex128; real
        taps belong to ``per_channel_arbitrary``.  Rate, N𝜙, state and call length are shared, only the two filter banks differ;
        channel c is bit for bit ``FIRFilter.complex_taps_arbitrary(H[c], rate, Nphi)`` fed ``x[c]`` (include/multirate_hip.h:
        per-channel complex taps for FIRArbitrary).  The output is always complex (Complex128 if either side is 64-bit); STRICT
        numerics only.  The filter binds to exactly ``H.shape[0]`` channels; ``taps(which)`` has shape (nchannels, tapsPer𝜙, N𝜙)
        and ``tapsforphase`` (nchannels, tapsPer𝜙), both complex.  The device object is created by
        ``mrhip_create_arbitrary_bank_ctaps``."""
        who = "per_channel_complex_taps_arbitrary"
        _takes_rate(rate, who, "per_channel_complex_taps")
        H = _complex_taps(_tap_matrix(H, who), who, "per_channel_arbitrary")
        return cls._of_bank(H, float(rate), int(Nphi), device=device, _complex_taps=True)

    @classmethod
    def per_channel_farrow(cls, H, rate, Nphi: int = 32, polyorder=4, *, device: int = 0, numerics: int = NUMERICS_STRICT):
        """One FIRFilter(H[c], rate::Float, N𝜙, polyorder) per channel behind one filter object: FIRFarrow with per-channel taps (a
        per-antenna equaliser or per-sensor calibration filter in front of a common, continuously variable rate change).  ``H``: shape
        (nchannels, hLen), Float32 or Float64.  The phase schedule does not depend on the taps: rate, N𝜙, polyorder, state and call
        length are shared, only the polynomial banks differ (every row is fitted on its own); channel c is bit for bit
        ``FIRFilter(H[c], rate, Nphi, polyorder)`` fed ``x[c]``, under STRICT and FUSED (include/multirate_hip.h: per-channel taps
        for FIRFarrow).  The filter binds to exactly ``H.shape[0]`` channels; ``pnfb()`` has shape (nchannels, tapsPer𝜙, polyorder+1)
        and ``tapsforphase`` (nchannels, tapsPer𝜙).  A caller-fitted ``pnfb`` is not accepted here.  The device object is created by
        ``mrhip_create_farrow_bank``."""
        _takes_rate(rate, "per_channel_farrow", "per_channel")
        _takes_polyorder(polyorder, "per_channel_farrow", "per_channel_arbitrary")
        H = _tap_matrix(_real_taps(H, "per_channel_farrow", "complex taps: FIRFilter.per_channel_complex_taps_farrow"), "per_channel_farrow")
        return cls._of_bank(_as_taps(H), float(rate), int(Nphi), int(polyorder), device=device, numerics=numerics)

    @classmethod
    def per_channel_complex_taps_farrow(cls, H, rate, Nphi: int = 32, polyorder=4, *, device: int = 0):
        """One FIRFilter(H[c]::Vector{Complex64 / Complex128}, rate::Float, N𝜙, polyorder) per channel behind one filter object:
        FIRFarrow with per-channel complex taps (a prototype rotated to every channel's own centre frequency, or a per-antenna complex
        equaliser, in front of a common, continuously variable rate change).  ``H``: shape (nchannels, hLen), Complex64 or
        Complex128; real taps belong to ``per_channel_farrow``.  Rate, N𝜙, polyorder, state and call length are shared, only the
        polynomial banks differ (every row is fitted on its own, per component); channel c is bit for bit
        ``FIRFilter.complex_taps_farrow(H[c], rate, Nphi, polyorder)`` fed ``x[c]`` (include/multirate_hip.h: per-channel complex taps
        for FIRFarrow).  The output is always complex (Complex128 if either side is 64-bit); STRICT numerics only.  The filter binds
        to exactly ``H.shape[0]`` channels; ``pnfb()`` has shape (nchannels, tapsPer𝜙, polyorder+1) and ``tapsforphase``
        (nchannels, tapsPer𝜙), both complex.  A caller-fitted ``pnfb`` is not accepted here.  The device object is created by
        ``mrhip_create_farrow_bank_ctaps``."""
        who = "per_channel_complex_taps_farrow"
        _takes_rate(rate, who, "per_channel_complex_taps")
        _takes_polyorder(polyorder, who, "per_channel_complex_taps_arbitrary")
        H = _complex_taps(_tap_matrix(H, who), who, "per_channel_farrow")
        return cls._of_bank(H, float(rate), int(Nphi), int(polyorder), device=device, _complex_taps=True)

    @classmethod
    def _of_bank(cls, H, *args, **kwargs):
        """the filter of row 0 of the (nchannels, hLen) matrix, with the matrix behind it"""
        H = np.ascontiguousarray(H)
        f = cls(H[0], *args, **kwargs)
        f._bank = H.copy()
        return f

    # -- lifetime
    def _ensure(self, tx: np.dtype, nch: int):
        tx = np.dtype(tx)
        if self._handle is not None:
            if tx != self._tx or nch != self._nch:
                raise MultirateHIPError(1, f"filter was bound to {self._nch} channel(s) of {self._tx}; "
                                           f"got {nch} of {tx}")
            return
        if tx not in _NP2DT:
            raise MultirateHIPError(1, f"unsupported sample dtype {tx}")
        for mirror, call in ((self._rates, "set_channel_rates_device"), (self._chan_taps, "set_channel_taps_device"), (self._chan_farrow, "set_channel_pnfb_ctaps_device" if self._farrow_ctaps else "set_channel_pnfb_device"),
                             (self._chan_ctaps, "set_channel_ctaps_device")):
            if isinstance(mirror, _DeviceResident):
                raise MultirateHIPError(1, f"the filter was closed after {call}: its values lived on the device and are gone; install new ones "
                                           f"through the host call before binding again")
        out = C.c_void_p()
        if self._bank is not None and nch != self._bank.shape[0]:
            raise MultirateHIPError(1, f"a per-channel filter of {self._bank.shape[0]} tap vectors binds to exactly that many channels; got {nch}")
        if self._rates is not None and nch != len(self._rates):
            raise MultirateHIPError(1, f"a filter of {len(self._rates)} per-channel rates binds to exactly that many channels; got {nch}")
        # the entry point follows from what the object holds: family, then _bank or _rates, _pnfb for a bank handed in, _ctaps for
        # complex taps (mrhip_create_rational itself takes both tap classes)
        family = {ARBITRARY: "arbitrary", FARROW: "farrow"}.get(self.kind, "rational")
        taps = self.h if self._bank is None else self._bank
        name = "mrhip_create_" + family + ("_bank" if self._bank is not None else "_rates" if self._rates is not None else "")
        first = taps
        if self.kind == FARROW and self._pnfb_in is not None and self._bank is None:
            name, first = name + "_pnfb", self._pnfb_in
        if taps.dtype.kind == "c" and name != "mrhip_create_rational":
            name += "_ctaps"
        if family == "rational":
            middle = (self.ratio.numerator, self.ratio.denominator)
        else:
            middle = (self.rate if self._rates is None else _ptr(self._rates), self.Nphi) + ((self.polyorder,) if self.kind == FARROW else ())
        rc = getattr(self._lib, name)(_ptr(first), taps.shape[-1], _NP2DT[taps.dtype], *middle, _NP2DT[tx], nch, self.device, C.byref(out))
        _check(rc)
        self._handle, self._tx, self._nch = out, tx, nch
        if self.numerics != NUMERICS_STRICT:
            _check(self._lib.mrhip_set_numerics(self._handle, self.numerics))
        if self._chan_taps is not None:                              # (set_channel_taps on the unbound filter)
            _check(self._lib.mrhip_set_channel_taps(self._handle, _ptr(self._chan_taps), self._chan_taps.shape[1], _NP2DT[self._chan_taps.dtype]))
        if self._chan_farrow is not None:                            # (set_channel_taps_farrow / set_channel_pnfb on the unbound filter)
            self._install_chan_farrow(*self._chan_farrow)
        if self._chan_ctaps is not None:                             # (set_channel_ctaps on the unbound filter; after the real taps, if both were set)
            _check(self._lib.mrhip_set_channel_ctaps(self._handle, _ptr(self._chan_ctaps), self._chan_ctaps.shape[1], _NP2DT[self._chan_ctaps.dtype]))

    def _install_chan_farrow(self, what, M):
        if what == "taps":
            _check(self._lib.mrhip_set_channel_taps_farrow(self._handle, _ptr(M), M.shape[1], _NP2DT[M.dtype]))
        elif what == "ctaps":
            _check(self._lib.mrhip_set_channel_ctaps_farrow(self._handle, _ptr(M), M.shape[1], _NP2DT[M.dtype]))
        elif what == "cpnfb":                 # (complex128: (re, im) pairs of Float64, the C layout)
            _check(self._lib.mrhip_set_channel_pnfb_ctaps(self._handle, _ptr(M), M.shape[1], M.shape[2] - 1))
        else:
            _check(self._lib.mrhip_set_channel_pnfb(self._handle, _ptr(M), M.shape[1], M.shape[2] - 1))

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.mrhip_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- introspection
    @property
    def kernel_name(self) -> str:
        return KIND_NAMES[self.kind]

    @property
    def output_dtype(self):
        if self._tx is None:
            return None
        return _DT2NP[self._lib.mrhip_output_dtype(_NP2DT[self._tap_dtype], _NP2DT[self._tx])]

    @property
    def _tap_dtype(self):
        """the filter's tap type: that of ``h``, or the complex type of its precision once complex per-channel taps are installed
        (``set_channel_ctaps`` and its siblings on a filter of ``per_channel_rates``; ``set_channel_ctaps_farrow`` and its siblings on
        one of ``per_channel_rates_farrow``)"""
        if self._chan_ctaps is None and not self._farrow_ctaps:
            return self.h.dtype
        return np.dtype(np.complex128 if self.h.dtype == np.float64 else np.complex64)

    @property
    def state(self) -> _State:
        st = _State()
        if self._rates is not None:
            raise MultirateHIPError(5, "state: the filter has per-channel rates, so a state per channel -- use channel_states")
        if self._handle is None:  # constructor state, src/Filters.jl:77-78,110-115
            st.kind = self.kind
            st.phiIdx, st.inputDeficit, st.xIdx = 1, 1, 1
            st.phiAccumulator, st.alpha = 1.0, 0.0
            st.Nphi, st.tapsPerPhi, st.historyLen = self.Nphi, self.tapsPerPhi, self.historyLen
            st.interpolation, st.decimation, st.hLen = self.interpolation, self.decimation, len(self.h)
            st.rate = self.rate or 0.0
            st.delta = self.Nphi / self.rate if self.rate else 0.0
            return st
        _check(self._lib.mrhip_get_state(self._handle, C.byref(st)))
        return st

    def set_state(self, phiIdx: int = 1, inputDeficit: int = 1, phiAccumulator: float = 1.0):
        if self._handle is None:
            raise MultirateHIPError(1, "set_state needs a bound filter (call filt once, or bind())")
        _check(self._lib.mrhip_set_state(self._handle, phiIdx, inputDeficit, phiAccumulator))

    def bind(self, dtype, nchannels: int = 1):
        """Create the device object now (normally done by the first filt call)."""
        self._ensure(np.dtype(dtype), int(nchannels))
        return self

    @property
    def history(self) -> np.ndarray:
        """FIRFilter.history (src/Filters.jl:153); shape (historyLen,) or (nchannels, historyLen)."""
        if self._handle is None:
            return np.zeros(self.historyLen)
        out = np.zeros((self._nch, self.historyLen), dtype=self._tx)
        _check(self._lib.mrhip_get_history(self._handle, _ptr(out)))
        return out[0] if self._nch == 1 else out

    def set_history(self, hist):
        hist = np.ascontiguousarray(hist, dtype=self._tx).reshape(self._nch, self.historyLen)
        _check(self._lib.mrhip_set_history(self._handle, _ptr(hist)))

    def taps(self, which: int = 0) -> np.ndarray:
        """kernel.h (flipped) / kernel.pfb (which=0) or kernel.dpfb (which=1) as stored.  A per-channel filter: one bank per channel,
        shape (nchannels, tapsPer𝜙, N𝜙)."""
        if self._handle is None:
            raise MultirateHIPError(1, "taps() needs a bound filter")
        if self._bank is not None or self._chan_taps is not None or self._chan_ctaps is not None:
            out = np.zeros((self._nch, self.Nphi, self.tapsPerPhi), dtype=self._tap_dtype)
            _check(self._lib.mrhip_get_taps(self._handle, which, _ptr(out)))
            return out.transpose(0, 2, 1).copy()
        out = np.zeros(self.tapsPerPhi * self.Nphi, dtype=self.h.dtype)
        _check(self._lib.mrhip_get_taps(self._handle, which, _ptr(out)))
        return out.reshape(self.Nphi, self.tapsPerPhi).T.copy()

    def pnfb(self) -> np.ndarray:
        """FIRFarrow.pnfb (src/Filters.jl:126): tapsPer𝜙 polynomials, ascending powers, shape (tapsPer𝜙, polyorder+1); a per-channel
        filter (FIRFilter.per_channel_farrow; complex: FIRFilter.per_channel_complex_taps_farrow): (nchannels, tapsPer𝜙, polyorder+1)."""
        if self._handle is None or self.kind != FARROW:
            raise MultirateHIPError(1, "pnfb() needs a bound FIRFarrow filter")
        shape = (self.tapsPerPhi, self.polyorder + 1)
        out = np.zeros((self._nch,) + shape if self._bank is not None or self._chan_farrow is not None else shape, dtype=np.complex128 if self._tap_dtype.kind == "c" else np.float64)
        _check(self._lib.mrhip_get_pnfb(self._handle, _ptr(out)))
        return out

    def tapsforphase(self, phase: float) -> np.ndarray:
        """tapsforphase(kernel::FIRArbitrary, phase), src/Filters.jl:677-690, and
        tapsforphase(kernel::FIRFarrow, phase), src/Filters.jl:764-775."""
        if self._handle is None or self.kind not in (ARBITRARY, FARROW):
            raise MultirateHIPError(1, "tapsforphase() needs a bound FIRArbitrary or FIRFarrow filter")
        banks = self._bank is not None or ((self._chan_taps is not None or self._chan_ctaps is not None) and self.kind == ARBITRARY) or (self._chan_farrow is not None and self.kind == FARROW)
        rows = (self._nch, self.tapsPerPhi) if banks else self.tapsPerPhi   # (a per-channel filter: one row per channel)
        out = np.zeros(rows, dtype=self._tap_dtype)
        fn = self._lib.mrhip_farrow_tapsforphase if self.kind == FARROW else self._lib.mrhip_arbitrary_tapsforphase
        _check(fn(self._handle, float(phase), _ptr(out)))
        return out

    def setphase(self, phi: float):
        """setphase(self::FIRFilter, 𝜙), src/Filters.jl:210-235, 𝜙 in [0, 1].  The reference's methods for
        FIRInterpolator/FIRRational use an undefined variable (:212); the evident intent -- the phase index that
        corresponds to the fraction 𝜙 of one input sample -- is implemented: 𝜙Idx = floor(𝜙*N𝜙) + 1, clipped to
        N𝜙.  FIRArbitrary: (α, 𝜙Idx) = modf(𝜙*N𝜙) as written (:217-222), stored as 𝜙Accumulator = 𝜙Idx + α clipped
        to [1, N𝜙+1).  FIRFarrow: 𝜙Idx = 𝜙*(N𝜙-1)+1 (:226)."""
        if not 0.0 <= phi <= 1.0:
            raise MultirateHIPError(1, "phase must be in [0, 1]")            # @assert, :211
        if self._handle is None:
            raise MultirateHIPError(1, "setphase needs a bound filter (call filt once, or bind())")
        st = self.state
        if self.kind in (INTERPOLATOR, RATIONAL):
            idx = min(int(phi * self.Nphi) + 1, self.Nphi)
            self.set_state(idx, st.inputDeficit, 1.0)
            return idx
        if self.kind == ARBITRARY:
            import math
            alpha, idx = math.modf(phi * self.Nphi)
            acc = min(max(idx + alpha, 1.0), math.nextafter(self.Nphi + 1.0, 0.0))
            self.set_state(1, st.inputDeficit, acc)
            return idx, alpha
        if self.kind == FARROW:
            acc = phi * (self.Nphi - 1) + 1
            self.set_state(1, st.inputDeficit, acc)
            return acc
        raise MultirateHIPError(5, f"setphase is not defined for {self.kernel_name}")

    def set_mod_form(self, julia03: bool):
        """FIRArbitrary / FIRFarrow: update()'s mod() (src/Filters.jl:668) as rem(y + rem(x, y), y) -- Julia Base before 0.4 -- instead
        of the exact remainder (``mrhip_set_mod_form``); identical for a power-of-two N𝜙."""
        if self._handle is None:
            raise MultirateHIPError(1, "set_mod_form needs a bound filter (call filt once, or bind())")
        _check(self._lib.mrhip_set_mod_form(self._handle, 1 if julia03 else 0))

    def set_timing(self, enabled=True):
        """True/False, or an int n > 1 to bracket every n-th compute launch only."""
        _check(self._lib.mrhip_set_timing(self._handle, int(enabled)))

    def timing_read(self):
        """(number of compute-kernel launches since the last read, sum of their durations in ms)."""
        n, ms = C.c_int64(0), C.c_double(0.0)
        _check(self._lib.mrhip_timing_read(self._handle, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def last_kernel_name(self) -> str:
        return self._lib.mrhip_last_kernel_name(self._handle).decode()

    def schedule_info(self) -> dict:
        """How the phase schedule of this FIRArbitrary / FIRFarrow filter (update(), src/Filters.jl:663-673) has been
        evaluated so far: on the device, by the closed form of a detected cycle, or by the host's serial loop."""
        v = (C.c_int64 * 8)()
        _check(self._lib.mrhip_schedule_info(self._handle, v, 8))
        keys = ("device_ok", "ncand", "nwin", "period", "host_steps", "periodic_steps", "device_pieces", "fallback_pieces")
        return dict(zip(keys, (int(a) for a in v)))

    # -- bookkeeping (src/Filters.jl:352-422)
    def outputlength(self, inputlength: int) -> int:
        if self._handle is None:
            self_state = self.state
            if self.kind == STANDARD:
                return inputlength
            if self.kind == INTERPOLATOR:
                return self.interpolation * inputlength
            if self.kind in (ARBITRARY, FARROW):
                import math
                return int(math.ceil((inputlength - self_state.inputDeficit + 1) * self.rate))
            return self._lib.mrhip_outputlength_ratio(inputlength, self.interpolation, self.decimation, 1)
        return self._lib.mrhip_outputlength(self._handle, inputlength)

    def inputlength(self, outputlength: int) -> int:
        if self._handle is None:
            if self.kind in (ARBITRARY, FARROW):
                raise MultirateHIPError(5, "inputlength is not defined for FIRArbitrary in the reference")
            return self._lib.mrhip_inputlength_ratio(outputlength, self.interpolation, self.decimation, 1)
        n = self._lib.mrhip_inputlength(self._handle, outputlength)
        if n < 0:
            raise MultirateHIPError(5, "inputlength is not defined for FIRArbitrary in the reference")
        return n

    def advance_state(self, inputlength: int) -> int:
        """Advance the stream state as a ``filt`` call over ``inputlength`` samples would, without data and without
        touching the history; returns the outputs that call would have written (``mrhip_advance_state``)."""
        if self._handle is None:
            raise MultirateHIPError(1, "advance_state needs a bound filter (call filt once, or bind())")
        n = self._lib.mrhip_advance_state(self._handle, int(inputlength))
        if n < 0:
            raise MultirateHIPError(1, self._lib.mrhip_last_error().decode("utf-8", "replace"))
        return n

    def next_output_count(self, inputlength: int) -> int:
        if self._handle is None:
            raise MultirateHIPError(1, "next_output_count needs a bound filter")
        return self._lib.mrhip_next_output_count(self._handle, inputlength)

    def reset(self):
        """reset(self::FIRFilter), src/Filters.jl:256-260."""
        if self._handle is not None:
            _check(self._lib.mrhip_reset(self._handle))
        return self

    # -- the hot path
    def _shape(self, x):
        if x.ndim == 1:
            return 1, x.shape[0], True
        if x.ndim == 2:
            return x.shape[0], x.shape[1], False
        raise MultirateHIPError(1, "x must be (n,) or (nchannels, n)")

    def filt_into(self, buffer, x, lengths=None) -> int:
        """filt!(buffer, self, x): writes per-channel outputs into ``buffer`` (same container kind as
        ``x``), returns the per-channel output count.  A filter with per-channel rates (``per_channel_rates``): torch device tensors
        only; ``buffer`` needs ``outputlength_bound(n)`` samples per row, row c receives its first ``counts[c]`` elements and nothing
        else, and the int64 counts of all channels are returned (after waiting for them).  ``lengths`` (such a filter only): one
        input length per channel -- channel c is fed ``x[c, :lengths[c]]``, ``x`` is the ``(nchannels, max_len)`` tensor and
        ``buffer`` needs ``outputlength_bound(max(lengths))`` per row (``mrhip_filt_device_rates_ragged``)."""
        if lengths is not None and self._rates is None:
            raise MultirateHIPError(1, "lengths needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        if self._rates is not None:
            counts = self._filt_into_rates(buffer, x, lengths=lengths)
            torch.cuda.current_stream(x.device).synchronize()
            return counts.cpu().numpy()
        nw = C.c_int64(0)
        if _is_torch(x):
            if not x.is_cuda:
                raise MultirateHIPError(1, "torch input must live on the GPU (use numpy for host data)")
            if x.stride(-1) != 1 or buffer.stride(-1) != 1:
                raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
            nch, n, _ = self._shape(x)
            self._ensure(_torch_np_dtype(x.dtype), nch)
            if _torch_np_dtype(buffer.dtype) != self.output_dtype:
                raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
            if x.device.index != self.device or buffer.device != x.device:
                raise MultirateHIPError(1, "x / buffer are not on the filter's device")
            cap = buffer.shape[-1]
            # channel strides in samples: views such as big[:, a:b] are filtered in place, no copy
            xs = x.stride(0) if x.ndim == 2 and nch > 1 else n
            ys = buffer.stride(0) if buffer.ndim == 2 and nch > 1 else cap
            if buffer.ndim != x.ndim or (x.ndim == 2 and buffer.shape[0] != nch):
                raise MultirateHIPError(1, "buffer must have one row per channel")
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _check(self._lib.mrhip_filt_device(self._handle, C.c_void_p(x.data_ptr()), n, xs,
                                               C.c_void_p(buffer.data_ptr()), cap, ys, C.byref(nw),
                                               C.c_void_p(stream)))
            return nw.value
        x = np.asarray(x)
        if not x.flags.c_contiguous:
            x = np.ascontiguousarray(x)
        nch, n, _ = self._shape(x)
        self._ensure(x.dtype, nch)
        if not isinstance(buffer, np.ndarray) or buffer.dtype != self.output_dtype or not buffer.flags.c_contiguous:
            raise MultirateHIPError(1, f"buffer must be a C-contiguous numpy array of {self.output_dtype}")
        cap = buffer.shape[-1]
        _check(self._lib.mrhip_filt_host(self._handle, _ptr(x), n, n, _ptr(buffer), cap, cap, C.byref(nw)))
        return nw.value

    def _rates_call_args(self, buffer, x, counts):
        """what the calls of a filter with per-channel rates share: the checks of x, buffer and counts, and (nchannels, samples per row,
        x stride, capacity, y stride, counts, stream)"""
        if not _is_torch(x) or not x.is_cuda or not _is_torch(buffer) or not buffer.is_cuda:
            raise MultirateHIPError(1, "a filter with per-channel rates takes torch device tensors")
        if (x.shape[-1] > 0 and x.stride(-1) != 1) or (buffer.shape[-1] > 0 and buffer.stride(-1) != 1):      # (an empty row has no stride to speak of)
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        nch, n, _ = self._shape(x)
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if _torch_np_dtype(buffer.dtype) != self.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
        if x.device.index != self.device or buffer.device != x.device:
            raise MultirateHIPError(1, "x / buffer are not on the filter's device")
        if buffer.ndim != x.ndim or (x.ndim == 2 and buffer.shape[0] != nch):
            raise MultirateHIPError(1, "buffer must have one row per channel")
        cap = buffer.shape[-1]
        xs = x.stride(0) if x.ndim == 2 and nch > 1 else n
        ys = buffer.stride(0) if buffer.ndim == 2 and nch > 1 else cap
        if counts is None:
            counts = torch.empty(nch, dtype=torch.int64, device=x.device)
        elif not (_is_torch(counts) and counts.is_cuda and counts.dtype == torch.int64 and counts.numel() >= nch and counts.is_contiguous()):
            raise MultirateHIPError(1, "counts must be a contiguous int64 CUDA tensor of nchannels elements")
        return nch, n, xs, cap, ys, counts, torch.cuda.current_stream(x.device).cuda_stream

    def _filt_into_rates(self, buffer, x, counts=None, lengths=None):
        """``mrhip_filt_device_rates`` (with ``lengths``: ``mrhip_filt_device_rates_ragged``) on torch's current stream; returns the
        int64 device tensor of the counts without waiting.  ``lengths`` may be reused as soon as the call returns."""
        nch, n, xs, cap, ys, counts, stream = self._rates_call_args(buffer, x, counts)
        if lengths is not None:
            lens = np.ascontiguousarray(lengths, dtype=np.int64)
            if lens.shape != (nch,):
                raise MultirateHIPError(1, f"lengths takes {nch} input lengths, one per channel; got shape {lens.shape}")
            if lens.size and int(lens.max()) > n:
                raise MultirateHIPError(1, f"a length of {int(lens.max())} exceeds the {n} samples a row of x holds")
            _check(self._lib.mrhip_filt_device_rates_ragged(self._handle, C.c_void_p(x.data_ptr()), _ptr(lens), xs, C.c_void_p(buffer.data_ptr()),
                                                            cap, ys, C.c_void_p(counts.data_ptr()), C.c_void_p(stream)))
            return counts
        _check(self._lib.mrhip_filt_device_rates(self._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()), cap, ys,
                                                 C.c_void_p(counts.data_ptr()), C.c_void_p(stream)))
        return counts

    def filt_rates_async(self, buffer, x, *, lengths=None, max_length=None, after=None, counts=None):
        """A call of a filter with per-channel rates whose input lengths the host never sees, enqueued on torch's current stream; returns
        the int64 device tensor of the counts WITHOUT waiting.  Exactly one of the two sources is given:

        ``lengths``: a CUDA int64 tensor of ``nchannels`` lengths, read in stream order (it may be produced by work enqueued just before
        the call and overwritten by work enqueued after it), with ``max_length``, the declared maximum of its values: ``buffer`` needs
        ``outputlength_bound(max_length)`` per row.  Channel c is fed ``x[c, :lengths[c]]``; a value outside ``[0, max_length]`` feeds
        the channel nothing in this call and makes ``channel_states`` raise until ``set_channel_states`` or ``reset()``
        (``mrhip_filt_device_rates_lens_device``).

        ``after=prev``: ``x`` is the buffer ``prev``'s latest call on this stream wrote, and the lengths are that call's counts, taken
        on the device -- per channel from a ``prev`` with per-channel rates, the one count of a one-state ``prev`` whose latest call was
        ``filt_into_async``.  ``max_length`` (default: the row length of ``x``) is ``prev.outputlength_bound`` of ``prev``'s (largest)
        input length (``mrhip_filt_device_rates_chained``)."""
        if self._rates is None:
            raise MultirateHIPError(1, "filt_rates_async needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        if (lengths is None) == (after is None):
            raise MultirateHIPError(1, "filt_rates_async takes exactly one of lengths (with max_length) and after")
        nrates = len(self._rates)
        if lengths is not None:
            if not _is_torch(lengths) or not lengths.is_cuda:
                raise MultirateHIPError(1, "filt_rates_async: lengths must be a CUDA tensor (host lengths go through filt_into(buffer, x, lengths))")
            if lengths.dtype != torch.int64:
                raise MultirateHIPError(1, f"filt_rates_async: lengths must be int64, got {lengths.dtype}")
            if tuple(lengths.shape) != (nrates,) or not lengths.is_contiguous():
                raise MultirateHIPError(1, f"filt_rates_async: lengths takes {nrates} contiguous values, one per channel; got shape {tuple(lengths.shape)}")
            if max_length is None or int(max_length) != max_length or max_length < 0:
                raise MultirateHIPError(1, "filt_rates_async: lengths comes with max_length, the declared maximum of its values (an integer >= 0)")
        else:
            if not isinstance(after, FIRFilter) or after._handle is None:
                raise MultirateHIPError(1, "filt_rates_async: after must be a bound FIRFilter whose latest call wrote x")
            if max_length is not None and (int(max_length) != max_length or max_length < 0):
                raise MultirateHIPError(1, "filt_rates_async: max_length must be an integer >= 0")
        nch, n, xs, cap, ys, counts, stream = self._rates_call_args(buffer, x, counts)
        bound = n if max_length is None else int(max_length)
        if bound > n:
            raise MultirateHIPError(1, f"filt_rates_async: max_length {bound} exceeds the {n} samples a row of x holds")
        if lengths is not None:
            if lengths.device != x.device:
                raise MultirateHIPError(1, "filt_rates_async: lengths is not on the filter's device")
            _check(self._lib.mrhip_filt_device_rates_lens_device(self._handle, C.c_void_p(x.data_ptr()), C.c_void_p(lengths.data_ptr()), bound, xs,
                                                                 C.c_void_p(buffer.data_ptr()), cap, ys, C.c_void_p(counts.data_ptr()),
                                                                 C.c_void_p(stream)))
        else:
            _check(self._lib.mrhip_filt_device_rates_chained(self._handle, after._handle, C.c_void_p(x.data_ptr()), bound, xs,
                                                             C.c_void_p(buffer.data_ptr()), cap, ys, C.c_void_p(counts.data_ptr()), C.c_void_p(stream)))
        return counts

    @property
    def channel_states(self):
        """The per-channel states of a filter with per-channel rates (``mrhip_get_channel_states``; waits for the filter's stream): a list
        of ``ChannelState`` (rate, delta, phiAccumulator, alpha, phiIdx, inputDeficit, xIdx, last_count).  Unbound: constructor states."""
        if self._rates is None:
            raise MultirateHIPError(1, "channel_states needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        out = (ChannelState * len(self._rates))()
        if self._handle is None and isinstance(self._rates, _DeviceResident):
            raise MultirateHIPError(1, "channel_states: the filter was closed after set_channel_rates_device; its rates lived on the device")
        if self._handle is None:                                   # constructor state, src/Filters.jl:110-115 (FIRFarrow: 141-144)
            for c, r in enumerate(self._rates):
                out[c] = ChannelState(float(r), self.Nphi / float(r), 1.0, 0.0, 1, 1, 1, 0)
            return list(out)
        _check(self._lib.mrhip_get_channel_states(self._handle, C.cast(out, C.c_void_p)))
        return list(out)

    def set_channel_states(self, inputDeficit, phiAccumulator):
        """Per-channel ``inputDeficit`` (>= 1) and ``phiAccumulator`` (in [1, N𝜙+1)); 𝜙Idx and α follow as update() derives them
        (``mrhip_set_channel_states``)."""
        if self._rates is None or self._handle is None:
            raise MultirateHIPError(1, "set_channel_states needs a bound filter of FIRFilter.per_channel_rates (bind(), or call filt once)")
        d = np.ascontiguousarray(inputDeficit, dtype=np.int64)
        a = np.ascontiguousarray(phiAccumulator, dtype=np.float64)
        if d.shape != (self._nch,) or a.shape != (self._nch,):
            raise MultirateHIPError(1, f"set_channel_states takes {self._nch} inputDeficit and {self._nch} phiAccumulator values")
        _check(self._lib.mrhip_set_channel_states(self._handle, _ptr(d), _ptr(a)))

    def set_channel_rates(self, rates):
        """New per-channel rates between calls (``mrhip_set_channel_rates``; waits for the filter's stream): rate and delta of every
        channel change, phiAccumulator, inputDeficit, history and taps stay, ``outputlength_bound`` follows the new largest rate.
        Channel c continues bit for bit as ``FIRFilter(h, rates[c], ...)`` given its state and history would.  ``reset()`` keeps the
        current rates.  Unbound: the filter will be created at the new rates."""
        if self._rates is None:
            raise MultirateHIPError(1, "set_channel_rates needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        r = self._checked_rates(rates, "set_channel_rates")
        if r.shape != self._rates.shape:
            raise MultirateHIPError(1, f"set_channel_rates takes {len(self._rates)} rates, one per channel; got {len(r)}")
        if self._handle is not None:
            _check(self._lib.mrhip_set_channel_rates(self._handle, _ptr(r)))
        self._rates, self.rate = r, float(r.max())

    def set_channel_taps(self, H):
        """Per-channel taps on a filter of ``per_channel_rates`` (``mrhip_set_channel_taps``; waits for the filter's stream): ``H`` has
        shape (nchannels, hLen) in the filter's tap dtype, row c replaces ``h`` for channel c.  phiAccumulator, inputDeficit, rates and
        history stay; channel c continues bit for bit as ``FIRFilter(H[c], rates[c], Nphi)`` given its state and history would.  The
        taps may change between calls (an adaptive equaliser); ``reset()`` keeps the current taps.  From then on ``taps(which)`` has
        shape (nchannels, tapsPer𝜙, N𝜙) and ``tapsforphase`` (nchannels, tapsPer𝜙).  Unbound: the taps are installed at ``bind``.
        FIRArbitrary only (``per_channel_rates_farrow``: status 5); complex taps: status 5."""
        if self._rates is None:
            raise MultirateHIPError(1, "set_channel_taps needs a filter of FIRFilter.per_channel_rates")
        if self.kind != ARBITRARY:
            raise MultirateHIPError(5, "set_channel_taps: FIRFarrow with per-channel taps and per-channel rates is not this call's (set_channel_taps_farrow or set_channel_pnfb; FIRFilter.per_channel_rates takes this call)")
        H = _tap_matrix(_real_taps(H, "set_channel_taps", "complex taps with per-channel rates are left out"), "set_channel_taps")
        if self._chan_ctaps is not None:
            raise MultirateHIPError(5, "set_channel_taps: the filter holds complex per-channel taps (set_channel_ctaps); going back to real taps is left out")
        if H.shape != (len(self._rates), len(self.h)):
            raise MultirateHIPError(1, f"set_channel_taps takes a {(len(self._rates), len(self.h))} matrix, one row of the filter's hLen taps per channel; got {H.shape}")
        if H.dtype != self.h.dtype:
            raise MultirateHIPError(1, f"set_channel_taps takes taps of the filter's tap dtype {self.h.dtype}; got {H.dtype}")
        H = np.ascontiguousarray(H).copy()
        if self._handle is not None:
            _check(self._lib.mrhip_set_channel_taps(self._handle, _ptr(H), H.shape[1], _NP2DT[H.dtype]))
        self._chan_taps = H

    def _takes_farrow_rates(self, who):
        if self._rates is not None and self.kind == ARBITRARY:
            raise MultirateHIPError(1, f"{who}: a filter of FIRFilter.per_channel_rates takes set_channel_taps")
        if self._rates is None or self.kind != FARROW:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates_farrow")

    def set_channel_taps_farrow(self, H):
        """Per-channel taps on a filter of ``per_channel_rates_farrow`` (``mrhip_set_channel_taps_farrow``; waits for the filter's
        stream): ``H`` has shape (nchannels, hLen) in the filter's tap dtype, row c replaces ``h`` for channel c and is fitted on its own,
        as ``per_channel_farrow`` fits its rows.  phiAccumulator, inputDeficit, rates and history stay; channel c continues bit for bit
        as ``FIRFilter(H[c], rates[c], Nphi, polyorder)`` given its state and history would.  The taps may change between calls;
        ``reset()`` keeps the current taps.  From then on ``pnfb()`` has shape (nchannels, tapsPer𝜙, polyorder+1) and ``tapsforphase``
        (nchannels, tapsPer𝜙).  Unbound: the taps are installed at ``bind``.  Complex taps: status 5."""
        who = "set_channel_taps_farrow"
        self._takes_farrow_rates(who)
        H = _tap_matrix(_real_taps(H, who, "complex taps with per-channel rates are left out"), who)
        if self._farrow_ctaps:
            raise MultirateHIPError(5, f"{who}: the filter holds complex per-channel taps (set_channel_ctaps_farrow, set_channel_pnfb_ctaps); going back to real taps is left out")
        if H.shape != (len(self._rates), len(self.h)):
            raise MultirateHIPError(1, f"{who} takes a {(len(self._rates), len(self.h))} matrix, one row of the filter's hLen taps per channel; got {H.shape}")
        if H.dtype != self.h.dtype:
            raise MultirateHIPError(1, f"{who} takes taps of the filter's tap dtype {self.h.dtype}; got {H.dtype}")
        H = np.ascontiguousarray(H).copy()
        if self._handle is not None:
            self._install_chan_farrow("taps", H)
        self._chan_farrow = ("taps", H)

    def set_channel_pnfb(self, PN):
        """Caller-fitted per-channel polynomial banks on a filter of ``per_channel_rates_farrow`` (``mrhip_set_channel_pnfb``; waits for
        the filter's stream): ``PN`` has shape (nchannels, tapsPer𝜙, polyorder+1), ascending powers, and is rounded to the filter's tap
        dtype as a handed-over ``pnfb`` is.  The path of a block-adaptive user who updates coefficients directly.  State, rates and
        history stay, the banks may change between calls, ``reset()`` keeps them; ``pnfb()`` and ``tapsforphase`` answer per channel
        from then on.  Unbound: the banks are installed at ``bind``.  Complex banks: status 5."""
        who = "set_channel_pnfb"
        self._takes_farrow_rates(who)
        PN = _real_taps(PN, who, "complex taps with per-channel rates are left out")
        if self._farrow_ctaps:
            raise MultirateHIPError(5, f"{who}: the filter holds complex per-channel taps (set_channel_ctaps_farrow, set_channel_pnfb_ctaps); going back to real taps is left out")
        want = (len(self._rates), self.tapsPerPhi, self.polyorder + 1)
        if PN.shape != want:
            raise MultirateHIPError(1, f"{who} takes banks of shape (nchannels, tapsPerPhi, polyorder+1) = {want}; got {PN.shape}")
        PN = np.ascontiguousarray(PN, dtype=np.float64).copy()
        if self._handle is not None:
            self._install_chan_farrow("pnfb", PN)
        self._chan_farrow = ("pnfb", PN)

    # -- device-resident updates (include/multirate_hip.h, "Device-resident updates for the filters with per-channel rates")
    def _device_update_args(self, who, t, dtype, shape):
        """the checks the three device calls share: a bound filter, a contiguous torch CUDA tensor on the filter's device of the dtype
        and shape the C call reads; returns torch's current stream on that device"""
        if not _is_torch(t) or not t.is_cuda:
            raise MultirateHIPError(1, f"{who} takes a torch CUDA tensor (host values: the call without _device)")
        if self._handle is None:
            raise MultirateHIPError(1, f"{who} needs a bound filter (bind(), or call filt once): the values are installed in stream order")
        if t.device.index != self.device:
            raise MultirateHIPError(1, f"{who}: the tensor is not on the filter's device")
        if t.dtype != _np_torch_dtype(np.dtype(dtype)):
            raise MultirateHIPError(1, f"{who} takes a tensor of {np.dtype(dtype)}; got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise MultirateHIPError(1, f"{who} takes a tensor of shape {tuple(shape)}; got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise MultirateHIPError(1, f"{who} takes a contiguous tensor")
        return torch.cuda.current_stream(t.device).cuda_stream

    def set_channel_rates_device(self, rates, lo, hi):
        """New per-channel rates from DEVICE memory (``mrhip_set_channel_rates_device``), enqueued on torch's current stream without any
        wait: ``rates`` is a contiguous float64 CUDA tensor of nchannels values, ``[lo, hi]`` the range the caller declares for them
        (finite, > 0, lo >= 2^-30).  A value that is finite and inside the range is installed as ``set_channel_rates`` installs it; any
        other leaves its channel at the old rate and makes ``channel_states`` raise code 1 until ``set_channel_states`` or ``reset``.
        ``rate`` and ``outputlength_bound`` follow ``hi``.  The Python mirror no longer knows the rates: ``channel_states`` asks the
        library, and the filter cannot be bound again after ``close()``."""
        who = "set_channel_rates_device"
        if self._rates is None:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        stream = self._device_update_args(who, rates, np.float64, (self._nch,))
        _check(self._lib.mrhip_set_channel_rates_device(self._handle, C.c_void_p(rates.data_ptr()), float(lo), float(hi), C.c_void_p(stream)))
        self._rates, self.rate = _DeviceResident((self._nch,)), float(hi)

    def set_channel_taps_device(self, H):
        """Per-channel taps from DEVICE memory on a filter of ``per_channel_rates`` (``mrhip_set_channel_taps_device``), enqueued on
        torch's current stream: ``H`` is a contiguous (nchannels, hLen) CUDA tensor in the filter's tap dtype.  The banks are built on
        the device, bit for bit those of ``set_channel_taps``.  The first call on a filter whose taps are still shared allocates the
        banks and waits once; every later call only enqueues a kernel.  ``taps()`` and ``tapsforphase`` read the banks back."""
        who = "set_channel_taps_device"
        if self._rates is None:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates")
        if self.kind != ARBITRARY:
            raise MultirateHIPError(1, f"{who}: a filter of FIRFilter.per_channel_rates_farrow takes set_channel_pnfb_device (the fit on the device is left out)")
        if self._chan_ctaps is not None:
            raise MultirateHIPError(5, f"{who}: the filter holds complex per-channel taps (set_channel_ctaps); going back to real taps is left out")
        stream = self._device_update_args(who, H, self.h.dtype, (len(self._rates), len(self.h)))
        _check(self._lib.mrhip_set_channel_taps_device(self._handle, C.c_void_p(H.data_ptr()), len(self.h), _NP2DT[self.h.dtype], C.c_void_p(stream)))
        self._chan_taps = _DeviceResident((self._nch, len(self.h)))

    def _takes_ctaps(self, who):
        """the filter checks of the complex per-channel tap calls, in the library's order: the filter kind, then (by the callers) the
        matrix, then the numerics"""
        if self._rates is not None and self.kind == FARROW:
            raise MultirateHIPError(5, f"{who}: complex taps with per-channel rates for FIRFarrow are left out")
        if self._rates is None or self.kind != ARBITRARY:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates")
        return np.dtype(np.complex128 if self.h.dtype == np.float64 else np.complex64)

    def set_channel_ctaps(self, H):
        """COMPLEX per-channel taps on a filter of ``per_channel_rates``, with or without earlier ``set_channel_taps``
        (``mrhip_set_channel_ctaps``; waits for the filter's stream): ``H`` has shape (nchannels, hLen) in the complex type of the
        filter's tap precision (complex64 on float32 taps, complex128 on float64 taps), row c replaces the taps of channel c -- a
        prototype rotated to the channel's own centre frequency beside the channel's own rate (Doppler: a time scale and a carrier
        offset).  phiAccumulator, inputDeficit, rates and history stay; channel c continues bit for bit as
        ``FIRFilter.complex_taps_arbitrary(H[c], rates[c], Nphi)`` given its state and history would (STRICT only: a FUSED filter is
        status 5).  From then on ``output_dtype`` is complex also over real samples, ``taps(which)`` has shape (nchannels, tapsPer𝜙, N𝜙)
        and ``tapsforphase`` (nchannels, tapsPer𝜙), both complex; the taps may change between calls; ``reset()`` keeps them; going back
        to real taps is status 5.  Unbound: the taps are installed at ``bind``."""
        who = "set_channel_ctaps"
        ct = self._takes_ctaps(who)
        H = _tap_matrix(np.asarray(H), who)
        if H.shape != (len(self._rates), len(self.h)):
            raise MultirateHIPError(1, f"{who} takes a {(len(self._rates), len(self.h))} matrix, one row of the filter's hLen taps per channel; got {H.shape}")
        if H.dtype.kind != "c":
            raise MultirateHIPError(1, f"{who} takes complex taps; real taps: set_channel_taps")
        if H.dtype != ct:
            raise MultirateHIPError(1, f"{who} takes taps of the complex type of the filter's tap precision, {ct}; got {H.dtype}")
        if self.numerics != NUMERICS_STRICT:
            raise MultirateHIPError(5, f"{who}: the filter is in FUSED numerics and no FUSED form is defined for complex taps")
        H = np.ascontiguousarray(H).copy()
        if self._handle is not None:
            _check(self._lib.mrhip_set_channel_ctaps(self._handle, _ptr(H), H.shape[1], _NP2DT[H.dtype]))
        self._chan_ctaps = H

    def set_channel_ctaps_device(self, H):
        """Complex per-channel taps from DEVICE memory on a filter of ``per_channel_rates`` (``mrhip_set_channel_ctaps_device``),
        enqueued on torch's current stream: ``H`` is a contiguous (nchannels, hLen) CUDA tensor in the complex type of the filter's tap
        precision.  Both banks are built on the device, bit for bit those of ``set_channel_ctaps``.  The first call on a filter that
        holds no complex banks yet allocates them and waits once; every later call only enqueues a kernel.  ``taps()`` and
        ``tapsforphase`` read the banks back."""
        who = "set_channel_ctaps_device"
        ct = self._takes_ctaps(who)
        stream = self._device_update_args(who, H, ct, (len(self._rates), len(self.h)))
        if self.numerics != NUMERICS_STRICT:
            raise MultirateHIPError(5, f"{who}: the filter is in FUSED numerics and no FUSED form is defined for complex taps")
        _check(self._lib.mrhip_set_channel_ctaps_device(self._handle, C.c_void_p(H.data_ptr()), len(self.h), _NP2DT[ct], C.c_void_p(stream)))
        self._chan_ctaps = _DeviceResident((self._nch, len(self.h)))

    def set_channel_pnfb_device(self, PN):
        """Per-channel polynomial banks from DEVICE memory on a filter of ``per_channel_rates_farrow``
        (``mrhip_set_channel_pnfb_device``), enqueued on torch's current stream: ``PN`` is a contiguous float64 CUDA tensor of shape
        (nchannels, tapsPer𝜙, polyorder+1), rounded to the filter's tap dtype on the device as ``set_channel_pnfb`` rounds on the host.
        Allocation and waiting as ``set_channel_taps_device``; ``pnfb()`` and ``tapsforphase`` read the banks back."""
        who = "set_channel_pnfb_device"
        if self._rates is not None and self.kind == ARBITRARY:
            raise MultirateHIPError(1, f"{who}: a filter of FIRFilter.per_channel_rates takes set_channel_taps_device")
        if self._rates is None or self.kind != FARROW:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates_farrow")
        if self._farrow_ctaps:
            raise MultirateHIPError(5, f"{who}: the filter holds complex per-channel taps (set_channel_ctaps_farrow, set_channel_pnfb_ctaps); going back to real taps is left out")
        shape = (len(self._rates), self.tapsPerPhi, self.polyorder + 1)
        stream = self._device_update_args(who, PN, np.float64, shape)
        _check(self._lib.mrhip_set_channel_pnfb_device(self._handle, C.c_void_p(PN.data_ptr()), self.tapsPerPhi, self.polyorder, C.c_void_p(stream)))
        self._chan_farrow = _DeviceResident(shape)

    # -- complex per-channel taps on a filter of per_channel_rates_farrow (include/multirate_hip.h, "Complex per-channel taps with
    # per-channel rates for FIRFarrow")
    def _takes_ctaps_farrow(self, who, arb_call="set_channel_ctaps"):
        """the filter checks of the complex FIRFarrow calls, in the library's order: the filter kind (``arb_call``: where a FIRArbitrary
        filter is pointed to), then (by the callers) the array, then the numerics"""
        if self._rates is not None and self.kind == ARBITRARY:
            raise MultirateHIPError(1, f"{who}: a filter of FIRFilter.per_channel_rates takes {arb_call}")
        if self._rates is None or self.kind != FARROW:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates_farrow")
        return np.dtype(np.complex128 if self.h.dtype == np.float64 else np.complex64)

    def _strict_for_ctaps(self, who):
        if self.numerics != NUMERICS_STRICT:
            raise MultirateHIPError(5, f"{who}: the filter is in FUSED numerics and no FUSED form is defined for complex taps")

    def set_channel_ctaps_farrow(self, H):
        """COMPLEX per-channel taps on a filter of ``per_channel_rates_farrow``, with or without earlier ``set_channel_taps_farrow`` /
        ``set_channel_pnfb`` (``mrhip_set_channel_ctaps_farrow``; waits for the filter's stream): ``H`` has shape (nchannels, hLen) in
        the complex type of the filter's tap precision, row c replaces the taps of channel c and is fitted on its own, per component,
        as ``per_channel_complex_taps_farrow`` fits its rows -- a matched pulse rotated to the channel's own frequency beside the
        channel's own, continuously variable rate (Doppler).  phiAccumulator, inputDeficit, rates and history stay; channel c
        continues bit for bit as ``FIRFilter.complex_taps_farrow(H[c], rates[c], Nphi, polyorder)`` given its state and history would
        (STRICT only: a FUSED filter is status 5).  From then on ``output_dtype`` is complex also over real samples, ``pnfb()`` has
        shape (nchannels, tapsPer𝜙, polyorder+1) and ``tapsforphase`` (nchannels, tapsPer𝜙), both complex; the taps may change
        between calls; ``reset()`` keeps them; going back to real taps is status 5.  Unbound: the taps are installed at ``bind``."""
        who = "set_channel_ctaps_farrow"
        ct = self._takes_ctaps_farrow(who)
        H = _tap_matrix(np.asarray(H), who)
        if H.shape != (len(self._rates), len(self.h)):
            raise MultirateHIPError(1, f"{who} takes a {(len(self._rates), len(self.h))} matrix, one row of the filter's hLen taps per channel; got {H.shape}")
        if H.dtype.kind != "c":
            raise MultirateHIPError(1, f"{who} takes complex taps; real taps: set_channel_taps_farrow")
        if H.dtype != ct:
            raise MultirateHIPError(1, f"{who} takes taps of the complex type of the filter's tap precision, {ct}; got {H.dtype}")
        self._strict_for_ctaps(who)
        H = np.ascontiguousarray(H).copy()
        if self._handle is not None:
            self._install_chan_farrow("ctaps", H)
        self._chan_farrow, self._farrow_ctaps = ("ctaps", H), True

    def set_channel_pnfb_ctaps(self, PN):
        """Caller-fitted COMPLEX per-channel polynomial banks on a filter of ``per_channel_rates_farrow``
        (``mrhip_set_channel_pnfb_ctaps``; waits for the filter's stream): ``PN`` is complex of shape (nchannels, tapsPer𝜙,
        polyorder+1), ascending powers; every component is rounded to the filter's tap precision as a handed-over complex ``pnfb``
        is.  The filter becomes complex64 over float32 taps and complex128 over float64 taps.  Everything else as
        ``set_channel_ctaps_farrow``."""
        who = "set_channel_pnfb_ctaps"
        self._takes_ctaps_farrow(who)
        PN = np.asarray(PN)
        want = (len(self._rates), self.tapsPerPhi, self.polyorder + 1)
        if PN.shape != want:
            raise MultirateHIPError(1, f"{who} takes banks of shape (nchannels, tapsPerPhi, polyorder+1) = {want}; got {PN.shape}")
        if PN.dtype.kind != "c":
            raise MultirateHIPError(1, f"{who} takes complex banks; real banks: set_channel_pnfb")
        self._strict_for_ctaps(who)
        PN = np.ascontiguousarray(PN, dtype=np.complex128).copy()
        if self._handle is not None:
            self._install_chan_farrow("cpnfb", PN)
        self._chan_farrow, self._farrow_ctaps = ("cpnfb", PN), True

    def set_channel_pnfb_ctaps_device(self, PN):
        """Complex per-channel polynomial banks from DEVICE memory on a filter of ``per_channel_rates_farrow``
        (``mrhip_set_channel_pnfb_ctaps_device``), enqueued on torch's current stream: ``PN`` is a contiguous complex128 CUDA tensor of
        shape (nchannels, tapsPer𝜙, polyorder+1), rounded per component to the filter's tap precision on the device as
        ``set_channel_pnfb_ctaps`` rounds on the host.  The first call on a filter that holds no complex banks yet allocates them and
        waits once; every later call only enqueues a kernel.  ``pnfb()`` and ``tapsforphase`` read the banks back."""
        who = "set_channel_pnfb_ctaps_device"
        self._takes_ctaps_farrow(who)
        shape = (len(self._rates), self.tapsPerPhi, self.polyorder + 1)
        stream = self._device_update_args(who, PN, np.complex128, shape)
        self._strict_for_ctaps(who)
        _check(self._lib.mrhip_set_channel_pnfb_ctaps_device(self._handle, C.c_void_p(PN.data_ptr()), self.tapsPerPhi, self.polyorder, C.c_void_p(stream)))
        self._chan_farrow, self._farrow_ctaps = _DeviceResident(shape), True

    # -- the FIRFarrow fit on the device (include/multirate_hip.h, "The FIRFarrow fit on the device for the filters with per-channel rates")
    def set_channel_taps_farrow_device(self, H):
        """Per-channel taps from DEVICE memory on a filter of ``per_channel_rates_farrow``, FITTED on the device
        (``mrhip_set_channel_taps_farrow_device``), enqueued on torch's current stream: ``H`` is a contiguous (nchannels, hLen) CUDA
        tensor in the filter's tap dtype -- what a block-LMS equaliser or a matched-pulse tracker leaves on the GPU.  The banks are bit
        for bit those of ``set_channel_taps_farrow`` with the same matrix.  The first call on a filter whose bank is still shared
        allocates the banks and waits once (the first of these calls also uploads the fit's table); every later call only enqueues a
        kernel.  ``pnfb()`` and ``tapsforphase`` read the banks back.  Nphi above 1024: status 5 (the host call takes those)."""
        who = "set_channel_taps_farrow_device"
        if self._rates is not None and self.kind == ARBITRARY:
            raise MultirateHIPError(1, f"{who}: a filter of FIRFilter.per_channel_rates takes set_channel_taps_device")
        if self._rates is None or self.kind != FARROW:
            raise MultirateHIPError(1, f"{who} needs a filter of FIRFilter.per_channel_rates_farrow")
        if self._farrow_ctaps:
            raise MultirateHIPError(5, f"{who}: the filter holds complex per-channel taps (set_channel_ctaps_farrow, set_channel_pnfb_ctaps); going back to real taps is left out")
        stream = self._device_update_args(who, H, self.h.dtype, (len(self._rates), len(self.h)))
        _check(self._lib.mrhip_set_channel_taps_farrow_device(self._handle, C.c_void_p(H.data_ptr()), len(self.h), _NP2DT[self.h.dtype], C.c_void_p(stream)))
        self._chan_farrow = _DeviceResident((len(self._rates), self.tapsPerPhi, self.polyorder + 1))

    def set_channel_ctaps_farrow_device(self, H):
        """COMPLEX per-channel taps from DEVICE memory on a filter of ``per_channel_rates_farrow``, fitted per component on the device
        (``mrhip_set_channel_ctaps_farrow_device``), enqueued on torch's current stream: ``H`` is a contiguous (nchannels, hLen) CUDA
        tensor in the complex type of the filter's tap precision.  The banks are bit for bit those of ``set_channel_ctaps_farrow``
        with the same matrix; the outputs are complex from then on, also over real samples (STRICT only: a FUSED filter is status 5).
        Allocation and waiting as ``set_channel_pnfb_ctaps_device``; ``pnfb()`` and ``tapsforphase`` read the banks back."""
        who = "set_channel_ctaps_farrow_device"
        ct = self._takes_ctaps_farrow(who, "set_channel_ctaps_device")
        stream = self._device_update_args(who, H, ct, (len(self._rates), len(self.h)))
        self._strict_for_ctaps(who)
        _check(self._lib.mrhip_set_channel_ctaps_farrow_device(self._handle, C.c_void_p(H.data_ptr()), len(self.h), _NP2DT[ct], C.c_void_p(stream)))
        self._chan_farrow, self._farrow_ctaps = _DeviceResident((len(self._rates), self.tapsPerPhi, self.polyorder + 1)), True

    def outputlength_bound(self, inputlength: int) -> int:
        """The largest per-channel output count a call of ``inputlength`` samples can have whatever the stream state
        (``mrhip_outputlength_bound``): the room ``filt_into_async`` -- and every call captured into a HIP graph -- needs."""
        if self._handle is None:
            raise MultirateHIPError(1, "outputlength_bound needs a bound filter (call filt once, or bind())")
        return self._lib.mrhip_outputlength_bound(self._handle, int(inputlength))

    def filt_into_async(self, buffer, x, count=None, after: "FIRFilter" = None) -> None:
        """filt!(buffer, self, x) planned ON THE DEVICE from the device-resident stream state (``mrhip_filt_device_async``):
        nothing is returned and the host never waits, so a loop of such calls only enqueues -- and captures into a HIP
        graph at any fixed chunk size, for every kind.  ``buffer`` must hold ``outputlength_bound(n)`` samples per channel;
        ``count`` (optional) is a one-element int64 CUDA tensor that receives the per-channel output count in stream order.
        ``sync_state()`` returns the last call's count and brings the host-side view of the state up to date.
        ``after=prev`` makes this a CHAINED call (``mrhip_filt_device_chained``): ``x`` is the buffer ``prev``'s latest
        asynchronous or captured call wrote, its length is that call's count (known on the device only) and ``x.shape[-1]`` is the
        bound the launch is sized for (``prev.outputlength_bound(...)``)."""
        if not _is_torch(x) or not x.is_cuda:
            raise MultirateHIPError(1, "filt_into_async takes torch device tensors")
        if x.stride(-1) != 1 or buffer.stride(-1) != 1:
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        nch, n, _ = self._shape(x)
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if _torch_np_dtype(buffer.dtype) != self.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
        if buffer.ndim != x.ndim or (x.ndim == 2 and buffer.shape[0] != nch):
            raise MultirateHIPError(1, "buffer must have one row per channel")
        cap = buffer.shape[-1]
        xs = x.stride(0) if x.ndim == 2 and nch > 1 else n
        ys = buffer.stride(0) if buffer.ndim == 2 and nch > 1 else cap
        cptr = None
        if count is not None:
            if not (_is_torch(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1):
                raise MultirateHIPError(1, "count must be an int64 CUDA tensor")
            cptr = C.c_void_p(count.data_ptr())
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if after is not None:
            if after._handle is None:
                raise MultirateHIPError(1, "after= needs a bound filter")
            _check(self._lib.mrhip_filt_device_chained(self._handle, after._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()),
                                                       cap, ys, cptr, C.c_void_p(stream)))
            return
        _check(self._lib.mrhip_filt_device_async(self._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()),
                                                 cap, ys, cptr, C.c_void_p(stream)))

    def sync_state(self) -> int:
        """Wait for the filter's enqueued calls (after a graph capture: for the device) and take the device-resident
        stream state over into the host object; returns the per-channel output count of the last call
        (``mrhip_sync_state``).  Raises if a device-planned call failed since the last ``sync_state``."""
        nw = C.c_int64(0)
        _check(self._lib.mrhip_sync_state(self._handle, C.byref(nw)))
        return nw.value

    def set_history_device(self, hist) -> None:
        """FIRFilter.history from a torch CUDA tensor, asynchronously on the current stream (``mrhip_set_history_device``)."""
        if not _is_torch(hist) or not hist.is_cuda or not hist.is_contiguous():
            raise MultirateHIPError(1, "set_history_device takes a contiguous torch CUDA tensor")
        if _torch_np_dtype(hist.dtype) != self._tx or hist.numel() != self._nch * self.historyLen:
            raise MultirateHIPError(1, f"history must hold {self._nch} x {self.historyLen} samples of {self._tx}")
        stream = torch.cuda.current_stream(hist.device).cuda_stream
        _check(self._lib.mrhip_set_history_device(self._handle, C.c_void_p(hist.data_ptr()), C.c_void_p(stream)))

    def filt_into_chunked(self, buffer, x, chunk: int) -> int:
        """The loop ``for a in range(0, n, chunk): filt!(buffer[k:], self, x[a:a+chunk])`` issued by the library in one
        call (torch device tensors only): streaming with the state carried on the device, bit-identical to the
        caller's own loop, without its per-call host overhead.  Returns the total per-channel output count."""
        if not _is_torch(x) or not x.is_cuda:
            raise MultirateHIPError(1, "filt_into_chunked takes torch device tensors")
        if x.stride(-1) != 1 or buffer.stride(-1) != 1:
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        nch, n, _ = self._shape(x)
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if _torch_np_dtype(buffer.dtype) != self.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
        cap = buffer.shape[-1]
        xs = x.stride(0) if x.ndim == 2 and nch > 1 else n
        ys = buffer.stride(0) if buffer.ndim == 2 and nch > 1 else cap
        nw = C.c_int64(0)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(self._lib.mrhip_filt_device_chunked(self._handle, C.c_void_p(x.data_ptr()), n, xs, int(chunk),
                                                   C.c_void_p(buffer.data_ptr()), cap, ys, C.byref(nw), C.c_void_p(stream)))
        return nw.value

    def open_ring(self, dtype=None, nchannels: int = None) -> "ChunkRing":
        """A ring of arriving chunks on this filter (``mrhip_ring_open``): one resident kernel instead of a launch per chunk.  The
        filter must be bound (``bind()`` / a first ``filt``), or ``dtype`` and ``nchannels`` given.  Use as a context manager."""
        if dtype is not None:
            self._ensure(np.dtype(dtype), int(nchannels or 1))
        if self._handle is None:
            raise MultirateHIPError(1, "open_ring needs a bound filter (bind(), or pass dtype and nchannels)")
        return ChunkRing(self)

    def filt(self, x, lengths=None):
        """filt(self, x): allocate the output, run filt!, trim to the samples written
        (src/Filters.jl:475,519,577,633,744).  ``lengths`` (a filter with per-channel rates only): channel c is fed
        ``x[c, :lengths[c]]``; the list of per-channel arrays is returned as without it."""
        if lengths is not None and self._rates is None:
            raise MultirateHIPError(1, "lengths needs a filter of FIRFilter.per_channel_rates or FIRFilter.per_channel_rates_farrow")
        # FIRArbitrary / FIRFarrow: like the reference (Filters.jl:744-752, 841-849) allocate the outputlength
        # estimate (+2: it is only a guess there) and trim to the count filt! returns -- the exact count would need
        # the whole serial phase recurrence up front, which the library instead pipelines with the kernels.
        if self._rates is not None:
            # per-channel rates: a list of nchannels arrays, each trimmed to its own count; numpy input goes to the device and back
            as_np = not _is_torch(x)
            if as_np:
                if torch is None:
                    raise MultirateHIPError(1, "a filter with per-channel rates takes torch device tensors")
                x = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{self.device}")
            nch, n, one = self._shape(x)
            self._ensure(_torch_np_dtype(x.dtype), nch)
            n_max = n if lengths is None else max(int(np.max(lengths, initial=0)), 0)
            y = torch.empty((nch, max(self.outputlength_bound(n_max), 0)), dtype=_np_torch_dtype(self.output_dtype), device=x.device)
            counts = self.filt_into(y[0] if one else y, x if x.stride(-1) == 1 else x.contiguous(), lengths)
            rows = [y[c, :int(counts[c])] for c in range(nch)]
            return [r.cpu().numpy() for r in rows] if as_np else rows
        est_mode = self.kind in (ARBITRARY, FARROW)
        if _is_torch(x):
            nch, n, one = self._shape(x)
            self._ensure(_torch_np_dtype(x.dtype), nch)
            cnt = max(self.outputlength(n), 0) + 2 if est_mode else max(self.next_output_count(n), 0)
            y = torch.empty((nch, cnt), dtype=_np_torch_dtype(self.output_dtype), device=x.device)
            got = 0
            if n > 0:
                got = self.filt_into(y[0] if one else y, x if x.stride(-1) == 1 else x.contiguous())
                assert est_mode or got == cnt
            if est_mode:
                y = y[:, :got]
            return y[0] if one else y
        x = np.ascontiguousarray(x)
        nch, n, one = self._shape(x)
        self._ensure(x.dtype, nch)
        cnt = max(self.outputlength(n), 0) + 2 if est_mode else max(self.next_output_count(n), 0)
        y = np.empty((nch, cnt), dtype=self.output_dtype)
        got = 0
        if n > 0:
            got = self.filt_into(y, x)
            assert est_mode or got == cnt
        if est_mode:
            y = np.ascontiguousarray(y[:, :got])
        return y[0] if one else y


class ChunkRing:
    """The reference's streaming loop ``for x_i in chunks: y_i = filt(self, x_i)`` (README.md:87-141) fed through a ring into ONE
    resident kernel (``mrhip_ring_*``): ``push(buffer, x)`` is ``filt!(buffer, self, x)`` for the next arriving chunk -- it returns
    the per-channel output count at once and the chunk's number; ``wait(seq)`` / ``drain()`` block until outputs are complete;
    ``close()`` hands the stream back to the filter.  ``x`` must be complete on the device when pushed (the resident kernel is not
    ordered behind any stream) and ``x`` / ``buffer`` must stay untouched until the chunk is complete."""

    def __init__(self, f: "FIRFilter"):
        self.filter = f
        self._lib = f._lib
        h = C.c_void_p()
        _check(self._lib.mrhip_ring_open(f._handle, C.byref(h)))
        self._h = h
        self._push = self._lib.mrhip_ring_push                   # (push_raw: no attribute look-ups, no byref objects per call)
        self._nw, self._seq = C.byref(C.c_int64(0)), C.byref(C.c_uint64(0))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        v = (C.c_int64 * 9)()
        _check(self._lib.mrhip_ring_info(self._h, v, 9))
        return {"resident": bool(v[0]), "depth": v[1], "pushed": v[2], "restarts": v[3], "steps_per_grab": v[4], "outputs_per_step": v[5],
                "shrunk": v[6], "workgroups": v[7], "xcds": v[8]}

    def _args(self, buffer, x):
        f = self.filter
        if not _is_torch(x) or not x.is_cuda or not _is_torch(buffer) or not buffer.is_cuda:
            raise MultirateHIPError(1, "a ring takes torch device tensors")
        if x.stride(-1) != 1 or buffer.stride(-1) != 1:
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        nch, n, _ = f._shape(x)
        if _torch_np_dtype(x.dtype) != f._tx or nch != f._nch:
            raise MultirateHIPError(1, "x does not match the sample type / channel count the filter is bound to")
        if _torch_np_dtype(buffer.dtype) != f.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {f.output_dtype}")
        if x.device.index != f.device or buffer.device != x.device:
            raise MultirateHIPError(1, "x / buffer are not on the filter's device")
        if buffer.ndim != x.ndim or (x.ndim == 2 and buffer.shape[0] != nch):
            raise MultirateHIPError(1, "buffer must have one row per channel")
        cap = buffer.shape[-1]
        xs = x.stride(0) if x.ndim == 2 and nch > 1 else n
        ys = buffer.stride(0) if buffer.ndim == 2 and nch > 1 else cap
        return n, xs, cap, ys

    def push(self, buffer, x):
        """filt!(buffer, self, x) for the next chunk: (per-channel output count, chunk number)"""
        n, xs, cap, ys = self._args(buffer, x)
        nw, seq = C.c_int64(0), C.c_uint64(0)
        _check(self._lib.mrhip_ring_push(self._h, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()), cap, ys, C.byref(nw), C.byref(seq)))
        return nw.value, seq.value

    def push_raw(self, x_ptr: int, n: int, x_stride: int, y_ptr: int, y_capacity: int, y_stride: int):
        """``push`` for a caller that already holds device addresses (a loop in another language, a preplanned stream): one
        ``mrhip_ring_push`` and nothing else -- no tensor checks; the same contract, unchecked: (count, chunk number)"""
        nw, seq = self._nw, self._seq
        _check(self._push(self._h, x_ptr, n, x_stride, y_ptr, y_capacity, y_stride, nw, seq))
        return nw._obj.value, seq._obj.value

    def push_chunks(self, buffer, x, chunk: int):
        """the library's loop of ``push`` over consecutive ``chunk``-sample pieces of a resident signal, outputs back to back in
        ``buffer``: (total per-channel output count, number of the last chunk)"""
        n, xs, cap, ys = self._args(buffer, x)
        nw, seq = C.c_int64(0), C.c_uint64(0)
        _check(self._lib.mrhip_ring_push_chunks(self._h, C.c_void_p(x.data_ptr()), n, xs, int(chunk), C.c_void_p(buffer.data_ptr()), cap, ys,
                                                C.byref(nw), C.byref(seq)))
        return nw.value, seq.value

    def wait(self, seq: int) -> None:
        _check(self._lib.mrhip_ring_wait(self._h, C.c_uint64(seq)))

    def drain(self) -> None:
        _check(self._lib.mrhip_ring_drain(self._h))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _check(self._lib.mrhip_ring_close(h))


class ShardedFIRFilter:
    """One FIRFilter whose channels are split over several GPUs of THIS process (``mrhip_sharded_*``; the one-process counterpart of
    sharding.py's one-rank-per-GPU ``ChannelShardedFilter``): shard i holds channels ``[start_i, start_i + count_i)`` on
    ``devices[i]``, no exchange during compute, one gather of the outputs at the end.

    ``filt(X)`` with a host (numpy) matrix ``(nchannels, n)`` filters every column split on all devices at once and returns the host
    result; ``filt_shards(xs)`` takes one CUDA tensor per shard (on that shard's device) and returns the per-shard outputs, which
    ``gather(ys, device)`` brings together on one device (peer copies)."""

    def __init__(self, h, ratio, nchannels: int, devices, *, Nphi: int = 32, polyorder=None, dtype=np.float32):
        self._lib = load_library()
        self.h = _as_taps(h)
        self._tx = np.dtype(dtype)
        self.nchannels = int(nchannels)
        self.devices = [int(d) for d in devices]
        ctor, num, den, rate = 0, 1, 1, 0.0
        if isinstance(ratio, float):
            ctor, rate = (2 if polyorder is not None else 1), float(ratio)
        else:
            r = Fraction(*ratio) if isinstance(ratio, tuple) else Fraction(ratio)
            num, den = r.numerator, r.denominator
        devs = (C.c_int * len(self.devices))(*self.devices)
        out = C.c_void_p()
        _check(self._lib.mrhip_sharded_create(ctor, _ptr(self.h), len(self.h), _NP2DT[self.h.dtype], num, den, rate, int(Nphi),
                                              int(polyorder or 0), _NP2DT[self._tx], self.nchannels, devs, len(self.devices), C.byref(out)))
        self._h = out
        self.output_dtype = _DT2NP[self._lib.mrhip_output_dtype(_NP2DT[self.h.dtype], _NP2DT[self._tx])]
        self.shards = []
        for i in range(self._lib.mrhip_sharded_nshards(self._h)):
            st, cnt, dev = C.c_int64(0), C.c_int64(0), C.c_int(0)
            _check(self._lib.mrhip_sharded_shard(self._h, i, C.byref(st), C.byref(cnt), C.byref(dev), None))
            self.shards.append((st.value, cnt.value, dev.value))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.mrhip_sharded_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(self._lib.mrhip_sharded_reset(self._h))
        return self

    def outputlength(self, n: int) -> int:
        return self._lib.mrhip_sharded_outputlength(self._h, int(n))

    def next_output_count(self, n: int) -> int:
        return self._lib.mrhip_sharded_next_output_count(self._h, int(n))

    def filt(self, X):
        """filt(self, X) for a host matrix with one channel per row: (nchannels, n) -> (nchannels, n_out)"""
        X = np.ascontiguousarray(X, dtype=self._tx)
        if X.ndim != 2 or X.shape[0] != self.nchannels:
            raise MultirateHIPError(1, f"X must be ({self.nchannels}, n)")
        n = X.shape[1]
        cap = max(self.outputlength(n), 0) + 2
        Y = np.empty((self.nchannels, cap), dtype=self.output_dtype)
        nw = C.c_int64(0)
        _check(self._lib.mrhip_sharded_filt_host(self._h, _ptr(X), n, n, _ptr(Y), cap, cap, C.byref(nw)))
        return np.ascontiguousarray(Y[:, :nw.value])

    def filt_shards(self, xs):
        """filt on device-resident data: xs[i] a (count_i, n) CUDA tensor on shard i's device; returns the per-shard outputs
        (asynchronous on the shards' streams: ``synchronize()`` or ``gather`` + ``synchronize()`` before reading)"""
        n = None
        for (st, cnt, dev), x in zip(self.shards, xs):
            if cnt and (not _is_torch(x) or not x.is_cuda or x.device.index != dev or x.shape != (cnt, x.shape[-1]) or x.stride(-1) != 1):
                raise MultirateHIPError(1, "xs[i] must be a (count_i, n) CUDA tensor on shard i's device")
            if cnt:
                n = x.shape[-1] if n is None else n
                if x.shape[-1] != n:
                    raise MultirateHIPError(1, "every shard takes the same number of samples per channel")
        cap = max(self.outputlength(n), 0) + 2
        ys = [torch.empty((cnt, cap), dtype=_np_torch_dtype(self.output_dtype), device=f"cuda:{dev}") if cnt else None for (st, cnt, dev) in self.shards]
        k = len(self.shards)
        xp = (C.c_void_p * k)(*[C.c_void_p(x.data_ptr()) if cnt else None for (st, cnt, dev), x in zip(self.shards, xs)])
        yp = (C.c_void_p * k)(*[C.c_void_p(y.data_ptr()) if y is not None else None for y in ys])
        xst = (C.c_int64 * k)(*[x.stride(0) if cnt else 0 for (st, cnt, dev), x in zip(self.shards, xs)])
        yst = (C.c_int64 * k)(*[cap] * k)
        nw = C.c_int64(0)
        # the shards run on private streams: each behind torch's current stream on its device (xs[i] may still be written there, ys[i]
        # came from the caching allocator in that stream's order) ...
        self._order(self._lib.mrhip_sharded_wait_stream)
        _check(self._lib.mrhip_sharded_filt_device(self._h, xp, n, xst, yp, cap, yst, C.byref(nw)))
        # ... and torch's stream behind them: later torch kernels see the outputs, the allocator may re-use ys[i] in stream order
        self._order(self._lib.mrhip_sharded_signal_stream)
        return [y[:, :nw.value] if y is not None else None for y in ys]

    def _order(self, fn):
        for i, (st, cnt, dev) in enumerate(self.shards):
            if cnt:
                _check(fn(self._h, i, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def gather(self, ys, device: int):
        """(nchannels, n_out) on ``device`` from the per-shard outputs (views as ``filt_shards`` returns them)"""
        n_out = next(y.shape[-1] for y in ys if y is not None)
        out = torch.empty((self.nchannels, n_out), dtype=_np_torch_dtype(self.output_dtype), device=f"cuda:{device}")
        k = len(self.shards)
        yp = (C.c_void_p * k)(*[C.c_void_p(y.data_ptr()) if y is not None else None for y in ys])
        yst = (C.c_int64 * k)(*[y.stride(0) if y is not None else 0 for y in ys])
        self._order(self._lib.mrhip_sharded_wait_stream)         # (ys may come from torch kernels; `out` from the allocator of its device:)
        for i, (st, cnt, dev) in enumerate(self.shards):
            if cnt and dev != int(device):
                # a shard on another device writes into `out`: behind the destination device's current stream too (an event recorded
                # there, waited for by the shard's stream -- HIP events order streams across devices)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(int(device)))
                with torch.cuda.device(dev):
                    torch.cuda.current_stream(dev).wait_event(ev)
                _check(self._lib.mrhip_sharded_wait_stream(self._h, i, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        _check(self._lib.mrhip_sharded_gather(self._h, yp, n_out, yst, C.c_void_p(out.data_ptr()), n_out, int(device)))
        self._order(self._lib.mrhip_sharded_signal_stream)
        for i, (st, cnt, dev) in enumerate(self.shards):         # the destination's stream behind every shard's copy
            if cnt and dev != int(device):
                ev = torch.cuda.Event()
                with torch.cuda.device(dev):
                    ev.record(torch.cuda.current_stream(dev))
                torch.cuda.current_stream(int(device)).wait_event(ev)
        return out

    def synchronize(self):
        _check(self._lib.mrhip_sharded_synchronize(self._h))


def filt_multi(filters, xs):
    """``[filt(f, x) for f, x in zip(filters, xs)]`` for INDEPENDENT FIRFilter objects (each its own phase, deficit, history
    and call length: the reference's one-FIRFilter-per-signal streaming usage, README.md:87-141) issued as ONE launch
    (``mrhip_filt_device_multi``).  ``xs`` are torch CUDA tensors, ``(n_i,)`` or ``(nchannels_i, n_i)``, contiguous."""
    if not filters or len(filters) != len(xs):
        raise MultirateHIPError(1, "filt_multi takes as many signals as filters")
    lib = load_library()
    n = len(filters)
    ys, shapes = [], []
    for f, x in zip(filters, xs):
        if not _is_torch(x) or not x.is_cuda or not x.is_contiguous():
            raise MultirateHIPError(1, "filt_multi takes contiguous torch CUDA tensors")
        nch, m, one = f._shape(x)
        f._ensure(_torch_np_dtype(x.dtype), nch)
        cnt = max(f.next_output_count(m), 0)
        ys.append(torch.empty((nch, cnt), dtype=_np_torch_dtype(f.output_dtype), device=x.device))
        shapes.append((m, cnt, one))
    hs = (C.c_void_p * n)(*[f._handle.value for f in filters])
    xp = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    yp = (C.c_void_p * n)(*[y.data_ptr() for y in ys])
    xl = (C.c_int64 * n)(*[s[0] for s in shapes])
    yc = (C.c_int64 * n)(*[s[1] for s in shapes])
    nw = (C.c_int64 * n)()
    stream = torch.cuda.current_stream(xs[0].device).cuda_stream
    _check(lib.mrhip_filt_device_multi(hs, n, xp, xl, yp, yc, nw, C.c_void_p(stream)))
    out = []
    for y, (m, cnt, one), got in zip(ys, shapes, nw):
        assert got == cnt
        out.append(y[0] if one else y)
    return out


class MultiStream:
    """A fixed set of independent FIRFilter streams and their (fixed) device buffers, prepared once so that every
    ``run()`` is ONE library call = one launch (``mrhip_filt_device_multi``): the per-round form of ``filt_multi`` for a
    loop over arriving chunks that land in the same buffers.  ``ys[i]`` must hold ``filters[i].next_output_count`` of every
    round (e.g. ``outputlength_bound``)."""

    def __init__(self, filters, ys, xs):
        self._lib = load_library()
        self.filters, self.ys, self.xs = list(filters), list(ys), list(xs)
        n = self.n = len(self.filters)
        for f, x in zip(self.filters, self.xs):
            nch, m, _ = f._shape(x)
            f._ensure(_torch_np_dtype(x.dtype), nch)
        self._hs = (C.c_void_p * n)(*[f._handle.value for f in self.filters])
        self._xp = (C.c_void_p * n)(*[x.data_ptr() for x in self.xs])
        self._yp = (C.c_void_p * n)(*[y.data_ptr() for y in self.ys])
        self._xl = (C.c_int64 * n)(*[x.shape[-1] for x in self.xs])
        self._yc = (C.c_int64 * n)(*[y.shape[-1] for y in self.ys])
        self.counts = (C.c_int64 * n)()

    def run(self):
        stream = torch.cuda.current_stream(self.xs[0].device).cuda_stream
        _check(self._lib.mrhip_filt_device_multi(self._hs, self.n, self._xp, self._xl, self._yp, self._yc, self.counts, C.c_void_p(stream)))
        return self.counts


# ---- free functions with the reference's names -------------------------------------------------
def filt(a, x, ratio=Fraction(1, 1), Nphi: int = 32, polyorder=None, **kw):
    """filt(self::FIRFilter, x)                                  src/Filters.jl:475,519,577,633,744,841
       filt(h::Vector, x::Vector, ratio::Rational)               src/Filters.jl:858-861
       filt(h::Vector, x::Vector, rate::Float, N𝜙)               src/Filters.jl:864-867
       filt(h::Vector, x::Vector, rate::Float, N𝜙, polyorder)    src/Filters.jl:870-873"""
    if isinstance(a, FIRFilter):
        return a.filt(x)
    f = FIRFilter(a, ratio, Nphi, polyorder, **kw)
    try:
        return f.filt(x)
    finally:
        f.close()


class FilterCascade:
    """Device-resident cascade (the reference chains ``filt`` calls by hand): ``filt`` runs the stages
    back to back on the current stream through the library's cascade object (``mrhip_cascade_*``) -- the intermediate
    signals live in device buffers the cascade owns and never leave HBM and, because every output count is
    closed-form on the host, nothing is read back between stages.  Each stage is an ordinary stateful FIRFilter, so
    chunked calls continue the stream exactly like calling the stages by hand (e.g. decimate 1//4, then 147//160).
    numpy inputs take the stages' host path one after the other."""

    def __init__(self, *stages: "FIRFilter"):
        if not stages or not all(isinstance(f, FIRFilter) for f in stages):
            raise MultirateHIPError(1, "FilterCascade takes one or more FIRFilter stages")
        self.stages = tuple(stages)
        self._lib = load_library()
        self._handle = None

    def _ensure(self, tx, nch: int):
        if self._handle is not None:
            # the bound cascade only knows the sample type and channel count of its first call: a later call with
            # another shape must raise like a lone FIRFilter does, not read or write past the caller's buffers
            self.stages[0]._ensure(np.dtype(tx), nch)
            return
        for f in self.stages:                      # stage i+1's sample type is stage i's output type
            f._ensure(np.dtype(tx), nch)
            tx = f.output_dtype
        arr = (C.c_void_p * len(self.stages))(*[f._handle for f in self.stages])
        out = C.c_void_p()
        _check(self._lib.mrhip_cascade_create(arr, len(self.stages), C.byref(out)))
        self._handle = out

    @property
    def output_dtype(self):
        return self.stages[-1].output_dtype

    def filt(self, x):
        if not _is_torch(x):
            for f in self.stages:
                x = f.filt(x)
            return x
        if not x.is_cuda:
            raise MultirateHIPError(1, "torch input must live on the GPU (use numpy for host data)")
        one = x.ndim == 1
        nch, n = (1, x.shape[0]) if one else (x.shape[0], x.shape[1])
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if x.stride(-1) != 1:
            x = x.contiguous()
        cnt = max(self._lib.mrhip_cascade_next_output_count(self._handle, n), 0)
        y = torch.empty((nch, cnt), dtype=_np_torch_dtype(self.output_dtype), device=x.device)
        nw = C.c_int64(0)
        xs = x.stride(0) if (not one and nch > 1) else n
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(self._lib.mrhip_cascade_filt_device(self._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(y.data_ptr()),
                                                   cnt, max(cnt, 1), C.byref(nw), C.c_void_p(stream)))
        assert nw.value == cnt
        return y[0] if one else y

    def filt_into(self, buffer, x) -> int:
        """The chain into a caller-owned device buffer (one row per channel); returns the per-channel output count.  This is
        the form a HIP graph can capture: every stage must then map its input length to the same count on every replay
        (inputlength * L a multiple of M), the buffer needs room for the last stage's ``outputlength_bound`` and one plain
        call of the same size must have run before (it allocates the buffers between the stages)."""
        if not (_is_torch(x) and x.is_cuda and _is_torch(buffer) and buffer.is_cuda):
            raise MultirateHIPError(1, "FilterCascade.filt_into takes device tensors")
        one = x.ndim == 1
        nch, n = (1, x.shape[0]) if one else (x.shape[0], x.shape[1])
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if x.stride(-1) != 1 or buffer.stride(-1) != 1:
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        if _torch_np_dtype(buffer.dtype) != self.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
        if buffer.ndim != x.ndim or (not one and buffer.shape[0] != nch):
            raise MultirateHIPError(1, "buffer must have one row per channel")
        cap = buffer.shape[-1]
        xs = x.stride(0) if (not one and nch > 1) else n
        ys = buffer.stride(0) if (not one and nch > 1) else cap
        nw = C.c_int64(0)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(self._lib.mrhip_cascade_filt_device(self._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()),
                                                   cap, ys, C.byref(nw), C.c_void_p(stream)))
        return nw.value

    def outputlength_bound(self, inputlength: int) -> int:
        """Room per channel an asynchronous (or captured) call of ``inputlength`` samples needs: the stages' bounds in turn."""
        n = int(inputlength)
        for f in self.stages:
            n = f.outputlength_bound(n)
        return n

    def filt_into_async(self, buffer, x, count=None) -> None:
        """The chain with nothing returned to the host (``mrhip_cascade_filt_device_async``): the first stage is planned on the
        device, every later one takes its input length from the previous stage's count ON THE DEVICE -- so the chain captures into a
        HIP graph at any chunk size.  ``buffer`` holds ``outputlength_bound(n)`` samples per channel; ``count``: one-element int64 CUDA
        tensor for the chain's per-channel output count.  Before a capture run one plain call of the same size (buffers)."""
        if not (_is_torch(x) and x.is_cuda and _is_torch(buffer) and buffer.is_cuda):
            raise MultirateHIPError(1, "FilterCascade.filt_into_async takes device tensors")
        one = x.ndim == 1
        nch, n = (1, x.shape[0]) if one else (x.shape[0], x.shape[1])
        self._ensure(_torch_np_dtype(x.dtype), nch)
        if x.stride(-1) != 1 or buffer.stride(-1) != 1:
            raise MultirateHIPError(1, "x and buffer must be contiguous along time (planar channels)")
        if _torch_np_dtype(buffer.dtype) != self.output_dtype:
            raise MultirateHIPError(1, f"buffer dtype must be {self.output_dtype}")
        if buffer.ndim != x.ndim or (not one and buffer.shape[0] != nch):
            raise MultirateHIPError(1, "buffer must have one row per channel")
        cap = buffer.shape[-1]
        xs = x.stride(0) if (not one and nch > 1) else n
        ys = buffer.stride(0) if (not one and nch > 1) else cap
        cptr = None
        if count is not None:
            if not (_is_torch(count) and count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1):
                raise MultirateHIPError(1, "count must be an int64 CUDA tensor")
            cptr = C.c_void_p(count.data_ptr())
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(self._lib.mrhip_cascade_filt_device_async(self._handle, C.c_void_p(x.data_ptr()), n, xs, C.c_void_p(buffer.data_ptr()),
                                                         cap, ys, cptr, C.c_void_p(stream)))

    def outputlength(self, inputlength: int) -> int:
        n = int(inputlength)
        for f in self.stages:
            n = f.outputlength(n)
        return n

    def reset(self):
        for f in self.stages:
            f.reset()
        return self

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.mrhip_cascade_destroy(self._handle)
            self._handle = None
        for f in self.stages:
            f.close()

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                self._lib.mrhip_cascade_destroy(self._handle)
                self._handle = None
        except Exception:
            pass


def filt_(buffer, self: FIRFilter, x):
    """filt!(buffer, self, x).  Returns what the reference returns: ``buffer`` for FIRStandard /
    FIRInterpolator (src/Filters.jl:472,516), the number of samples written for FIRRational /
    FIRDecimator / FIRArbitrary (:574,:630,:741)."""
    n = self.filt_into(buffer, x)
    return buffer if self.kind in (STANDARD, INTERPOLATOR) else n


def outputlength(self: FIRFilter, inputlength: int) -> int:
    """outputlength(self::FIRFilter, inputlength), src/Filters.jl:383-385."""
    return self.outputlength(inputlength)


def inputlength(self: FIRFilter, outputlength: int) -> int:
    """inputlength(self::FIRFilter, outputlength), src/Filters.jl:403-422."""
    return self.inputlength(outputlength)


def reset(self: FIRFilter) -> FIRFilter:
    """reset(self::FIRFilter), src/Filters.jl:256-260."""
    return self.reset()


def setphase(self: FIRFilter, phi: float):
    """setphase(self::FIRFilter, 𝜙), src/Filters.jl:235."""
    return self.setphase(phi)


def tapsforphase(self: FIRFilter, phase: float) -> np.ndarray:
    """tapsforphase(kernel::FIRArbitrary, phase), src/Filters.jl:690; tapsforphase(kernel::FIRFarrow, phase), :775."""
    return self.tapsforphase(phase)
