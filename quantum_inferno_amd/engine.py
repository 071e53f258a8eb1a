"""
Batched GPU engine behind the reference-signature wrappers.

A `TfrPlan` owns one qi_plan (include/qi_tfr.h): record length n, arithmetic type, device, the
Gabor atom banks and the Stockwell band table.  Band selection is done here on the host in
float64 (scales_dyadic) and handed to the library as tables; everything that touches a panel
runs in libqi_tfr.so.  Signals are [channels, n]; panels are [channels, bands, n].

PyTorch is used for device memory and streams only.
"""
import collections
import contextlib
import ctypes as C
import operator
import os
import threading
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import scales_dyadic as scales

_EPI_SPAN = 1024  # time samples per epilogue workgroup (csrc/qi_common.hpp:kEpiSpan)


def _real_dtype(dtype):
    if dtype in (torch.float32, np.float32, "float32", "f32"):
        return torch.float32
    if dtype in (torch.float64, np.float64, "float64", "f64", float):
        return torch.float64
    raise TypeError(f"unsupported dtype {dtype}: float32 or float64")


def _complex_of(rdtype):
    return torch.complex64 if rdtype == torch.float32 else torch.complex128


def default_device():
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def as_signal(sig, device=None, dtype=None):
    """-> (tensor [C, n] on the GPU, was_numpy, was_1d).  float32 stays float32, everything else
    becomes float64 (the reference computes in float64)."""
    was_numpy = not isinstance(sig, torch.Tensor)
    if was_numpy:
        arr = np.asarray(sig)
        if arr.dtype != np.float32 and arr.dtype != np.float64:
            arr = arr.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(arr))
    else:
        t = sig
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
    if dtype is not None:
        t = t.to(_real_dtype(dtype))
    if device is None:
        device = t.device if t.is_cuda else default_device()
    t = t.to(device)
    was_1d = t.dim() == 1
    if was_1d:
        t = t.unsqueeze(0)
    if t.dim() != 2:
        raise ValueError(f"signal must be 1-D [n] or 2-D [channels, n], got shape {tuple(t.shape)}")
    return t.contiguous(), was_numpy, was_1d


def _log2_rows(x, eps=0.0):
    """log2(x + eps) of a [C, count] real device tensor through the library (qi_log2_offset) -- the small marginals too:
    PyTorch computes nothing on the path."""
    lib = _lib.require_gpu()
    x = x.contiguous()
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    _lib.call(lib.qi_log2_offset, x.device, _lib.dtype_code(x.dtype), x.device.index, _lib.ptr(x), _lib.ptr(out), x.shape[0],
              x.numel() // x.shape[0], float(eps), None)
    return out


@dataclass
class TfrResult:
    """Outputs of one transform call; every field is a device tensor or None."""

    frequency_hz: np.ndarray
    coef: Optional[torch.Tensor] = None  # [C, B, n] complex
    bits: Optional[torch.Tensor] = None  # [C, B, n] log2(|z| + eps)
    power_band: Optional[torch.Tensor] = None  # [C, B] float64, sum over time of P
    power_time: Optional[torch.Tensor] = None  # [C, n], sum over bands of P
    stats: Optional[torch.Tensor] = None  # [C, 4] float64: max P, sum P, sum P log2 P, 0
    power_scale: float = 1.0
    reduced: Optional[torch.Tensor] = None  # float64 buffer the three reductions are views of (dist.reduced_slots)
    pooled: Optional[dict] = None  # method -> [C, B, windows] pooled power strips (TfrPlan.pooled_strip, stream.py)

    @property
    def max_power(self):
        return self.stats[:, 0]

    @property
    def total_power(self):
        return self.stats[:, 1]

    @property
    def entropy_bits(self):
        """Total Shannon entropy sum(pdf * -log2(pdf)), pdf = P / sum(P), from the one-pass sums
        H = log2 S - (sum P log2 P) / S (tfr_info.py:203-236 without materialising the panel; the
        reference's eps64 inside the log changes H by < 1e-8 bits)."""
        s = self.stats[:, 1]
        return _log2_rows(self.stats[:, 1:2])[:, 0] - self.stats[:, 2] / s

    def power_per_band_bits(self):
        """log2(sum_t P + eps) - max   (tfr_info.py:93)."""
        b = _log2_rows(self.power_band, float(scales.EPSILON64))
        return b - b.max(dim=1, keepdim=True).values

    def power_per_time_bits(self):
        """log2(sum_j P + eps) - max   (tfr_info.py:91)."""
        b = _log2_rows(self.power_time.to(torch.float64), float(scales.EPSILON64))
        return b - b.max(dim=1, keepdim=True).values


def out_descriptor(res, eps):
    """The C-ABI descriptor of the outputs `res` (a TfrResult) holds buffers for, at its power_scale."""
    return _lib.TfrOut(coef=_lib.ptr(res.coef), bits=_lib.ptr(res.bits), power_band=_lib.ptr(res.power_band),
                       power_time=_lib.ptr(res.power_time), stats=_lib.ptr(res.stats), power_scale=float(res.power_scale),
                       eps=float(eps))


def check_pooled_methods(methods, name="pooled_methods"):
    """-> the tuple of the pooling methods the device folds beside a transform, or the ValueError of another choice."""
    methods = tuple(methods)
    if not methods or any(m not in ("average", "max") for m in methods) or len(set(methods)) != len(methods):
        raise ValueError(f'{name} must be a subset of ("average", "max"), got {methods!r}')
    return methods


def reduced_views(n_ch, n_b, n, rdtype, device, reductions=True, reduced_out=None):
    """(reduced, power_band [C, B] f64, power_time [C, n], stats [C, 4] f64) of one transform: views into ONE float64 buffer
    for the whole reduced product (the message of dist.gather_reduced; layout dist.reduced_slots), new or the caller's
    `reduced_out` (e.g. a slice of one buffer for several transforms).  reductions="band": band powers and statistics only,
    no per-time marginal -- the kernels then write (and the tails read) no per-time planes at all, what a streaming job that
    keeps no per-time power asks for (stream.py); that form has no gather layout (reduced is None)."""
    from .dist import reduced_slots

    if reductions == "band":
        if reduced_out is not None:
            raise ValueError('reductions="band" has no gather layout: reduced_out does not apply')
        small = torch.empty(n_ch * (n_b + 4), dtype=torch.float64, device=device)
        return None, small[: n_ch * n_b].view(n_ch, n_b), None, small[n_ch * n_b :].view(n_ch, 4)
    slots = reduced_slots(n_ch, n_b, n, rdtype)
    if reduced_out is not None:
        if reduced_out.dtype != torch.float64 or reduced_out.numel() != slots or not reduced_out.is_contiguous():
            raise ValueError(f"reduced_out must be a contiguous float64 tensor of {slots} elements")
        reduced = reduced_out
    else:
        reduced = torch.empty(slots, dtype=torch.float64, device=device)
    o1 = reduced.numel() - n_ch * (n_b + 4)
    o2 = o1 + n_ch * n_b
    return (reduced, reduced[o1:o2].view(n_ch, n_b), reduced[:o1].view(rdtype)[: n_ch * n].view(n_ch, n),
            reduced[o2:].view(n_ch, 4))


def styx_bank_tables(order, n, fs, dictionary_type="norm"):
    """Host float64 tables of the styx_cwt Gabor bank (styx_cwt.py:29-40,68-144):
    returns (f_hz, p_re, p_im, omega, amp, scale)."""
    f_hz = scales.log_frequency_hz_from_fft_points(fs, n, order)
    scale, omega = scales.scale_from_frequency_hz(order, f_hz, fs)
    amp_norm = (np.pi * scale ** 2) ** (-1 / 4)
    if dictionary_type == "spect":
        amp = (4 * np.pi * scale ** 2) ** (-1 / 4) * amp_norm
    elif dictionary_type == "unit":
        amp = np.ones(scale.shape)
    else:
        amp = amp_norm
    return f_hz, 0.5 / scale ** 2, np.zeros_like(scale), omega, amp, scale


class TfrPlan:
    """GPU plan for records of n samples."""

    def __init__(self, n, dtype=torch.float32, device=None, workspace_bytes=None, engine=_lib.QI_ENGINE_AUTO):
        self._lib = _lib.require_gpu()
        self.n = int(n)
        self.rdtype = _real_dtype(dtype)
        self.device = torch.device(device) if device is not None else default_device()
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.workspace_bytes = int(workspace_bytes) if workspace_bytes else 0
        self._handle = C.c_void_p()
        if os.environ.get("QI_FORCE_HIPFFT"):  # testing aid: run everything on the hipFFT engine
            engine = _lib.QI_ENGINE_HIPFFT
        desc = _lib.PlanDesc(
            n=self.n,
            dtype=_lib.dtype_code(self.rdtype),
            device=self.device.index,
            engine=engine,
            flags=0,
            workspace_bytes=self.workspace_bytes,
        )
        _lib.check(self._lib.qi_plan_create(C.byref(self._handle), C.byref(desc)))
        self.freq = {}  # bank name -> host band centre frequencies
        self._stage = None  # staging panel of pooled(), kept between calls

    # -- sizing -------------------------------------------------------------------------------
    @staticmethod
    def workspace_for(n, n_bands, dtype, channels=1, cap_bytes=8 << 30):
        """Scratch that lets `channels` records of an n_bands panel go through in one tile."""
        esz = 16 if _real_dtype(dtype) == torch.float64 else 8
        length = 2 * n if (n & (n - 1)) == 0 else 1 << (2 * n - 2).bit_length()
        nblk = -(-n // _EPI_SPAN)
        # (a record's spectrum and one row per band; the native engines need the spectrum, one more row -- the staging slot
        # of their forward transform -- and the coarse planes of the zoom bands, which a table of ONE band would not leave)
        per_chan = (max(n_bands, 2) + 1) * length * esz + n_bands * nblk * 32 + 4096
        build = min(n_bands, 16) * length * 16
        need = max(per_chan * channels, build, 1 << 24)
        return int(min(max(need, per_chan), max(cap_bytes, per_chan)))

    # -- tables -------------------------------------------------------------------------------
    def _stream(self):
        return _lib.stream_ptr(self.device)

    def set_gabor_bank(self, which, f_hz, p_re, p_im, omega, amp):
        keep = [_lib.darr(a) for a in (p_re, p_im, omega, amp)]
        with torch.cuda.device(self.device):
            _lib.check(
                self._lib.qi_plan_set_gabor_bank(
                    self._handle, which, len(keep[0][0]), keep[0][1], keep[1][1], keep[2][1], keep[3][1], self._stream()
                )
            )
        self.freq[which] = np.asarray(f_hz)

    def set_styx_bank(self, order, fs, dictionary_type="norm"):
        f_hz, p_re, p_im, omega, amp, _ = styx_bank_tables(order, self.n, fs, dictionary_type)
        self.set_gabor_bank(_lib.QI_BANK_STYX, f_hz, p_re, p_im, omega, amp)
        return f_hz

    def set_stx_bands(self, order, fs):
        """Band table of styx_stx.stx_complex_any_scale_pow2 (styx_stx.py:207-219,233)."""
        f_hz = scales.log_frequency_hz_from_fft_points(fs, self.n, order)
        idx = scales.stx_shift_indices(f_hz, self.n, fs)
        sigma = scales.cycles_from_order(order) / (2 * np.pi * f_hz / fs)
        self.set_stx_table(f_hz, idx, sigma)
        return f_hz

    def set_stx_table(self, f_hz, shift_index, sigma):
        """Any Stockwell band table (qi_plan_set_stx_bands): shift index and Gaussian width in samples per band."""
        ia, ip = _lib.iarr(shift_index)
        sa, sp = _lib.darr(sigma)
        if len(ia) != len(sa):
            raise ValueError("shift_index and sigma must have one entry per band")
        _lib.check(self._lib.qi_plan_set_stx_bands(self._handle, len(ia), ip, sp))
        self.freq[_lib.QI_TABLE_STX] = np.asarray(f_hz)
        self.stx_index = ia

    # -- transforms ---------------------------------------------------------------------------
    # -- measurement --------------------------------------------------------------------------
    def profile(self, enable=True, stages=None, period=1):
        """Time stage launches with HIP events on the current stream (qi_plan_profile): every stage, or only the
        named ones (`stages`, names from `_lib.STAGES`), on every transform call or every `period`-th one -- each
        recorded event is a small bubble in the stream."""
        code = 1 if enable else 0
        if enable and stages is not None:
            code = 0
            for name in stages:
                code |= 1 << (_lib.STAGES.index(name) + 1)
        if enable and period > 1:
            code |= int(period) << 16
        _lib.check(self._lib.qi_plan_profile(self._handle, code))

    def stage_bands(self, stage):
        """Bands (over the styx, atoms and Stockwell tables) whose coefficients the kernels of `stage` produce."""
        k = _lib.STAGES.index(stage)
        return [int(self._lib.qi_plan_stage_bands(self._handle, which, k)) for which in (0, 1, 2)]

    def forward_low(self, which):
        """0 when the plan's native runs form the whole record spectrum; otherwise (low-bins forward transform) the power
        of two K with every spectrum bin table `which` reads inside (-K, K) (qi_plan_forward_low)."""
        return int(self._lib.qi_plan_forward_low(self._handle, which))

    def joint_planes(self, which):
        """Per-time planes table `which` (styx or Stockwell) writes in a joint one-record cwt_stx call (qi_plan_joint_planes);
        0 when the plan runs no joint call."""
        return int(self._lib.qi_plan_joint_planes(self._handle, which))

    def band_route(self, which, band, records=1):
        """(stage name, cls, run_cls, flags) of the kernels that produce row `band` of table `which` in a call of
        `records` records (qi_plan_band_route; the flag bits are _lib.ROUTE_*)."""
        r = _lib.BandRoute()
        _lib.check(self._lib.qi_plan_band_route(self._handle, which, int(band), int(records), C.byref(r)))
        return _lib.STAGES[r.stage], r.cls, r.run_cls, r.flags

    def profile_read(self):
        """{stage name: (total ms, launches)} since the last read (qi_plan_profile_read)."""
        ms = (C.c_double * len(_lib.STAGES))()
        cnt = (C.c_int64 * len(_lib.STAGES))()
        _lib.check(self._lib.qi_plan_profile_read(self._handle, ms, cnt, len(_lib.STAGES)))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_lib.STAGES)}

    def _signal(self, sig):
        if sig.dtype != self.rdtype or not sig.is_cuda or sig.device != self.device:
            sig = sig.to(device=self.device, dtype=self.rdtype)
        sig = sig.contiguous()
        if sig.dim() != 2 or sig.shape[1] != self.n:
            raise ValueError(f"signal must be [channels, {self.n}], got {tuple(sig.shape)}")
        return sig

    def _outputs(self, which, n_ch, coef, bits, reductions, power_scale, eps, out, reduced_out):
        """The TfrResult of one transform (new buffers, or those of `out`) and its C-ABI descriptor."""
        f_hz = self.freq.get(which)
        if f_hz is None:
            raise _lib.QiError("band table not set on this plan")
        n_b = len(f_hz)
        dev = self.device
        if out is not None:  # reuse the buffers of an earlier call of the same shape
            res = out
            if (res.coef is not None and res.coef.shape[0] != n_ch) or (res.stats is not None and res.stats.shape[0] != n_ch):
                raise ValueError("out= buffers were made for another channel count")
            res.power_scale = power_scale  # the reductions about to be written are those of this call's scale
        else:
            res = TfrResult(frequency_hz=f_hz, power_scale=power_scale)
            if coef:
                res.coef = torch.empty((n_ch, n_b, self.n), dtype=_complex_of(self.rdtype), device=dev)
            if bits:
                res.bits = torch.empty((n_ch, n_b, self.n), dtype=self.rdtype, device=dev)
            if reductions:
                res.reduced, res.power_band, res.power_time, res.stats = reduced_views(
                    n_ch, n_b, self.n, self.rdtype, dev, reductions, reduced_out)
        return res, out_descriptor(res, eps)

    def _run(self, which, sig, coef, bits, reductions, power_scale, eps, out=None, reduced_out=None):
        sig = self._signal(sig)
        n_ch = sig.shape[0]
        res, desc = self._outputs(which, n_ch, coef, bits, reductions, power_scale, eps, out, reduced_out)
        with torch.cuda.device(self.device):
            if which == _lib.QI_TABLE_STX:
                rc = self._lib.qi_stx(self._handle, _lib.ptr(sig), n_ch, C.byref(desc), self._stream())
            else:
                rc = self._lib.qi_cwt(self._handle, which, _lib.ptr(sig), n_ch, C.byref(desc), self._stream())
        _lib.check(rc)
        return res

    def cwt_stx(self, sig, coef=True, bits=False, reductions=False, power_scale=1.0, eps=0.0, out=None, reduced_out=None):
        """The styx CWT and the Stockwell transform of the same records in one call (qi_cwt_stx): (cwt, stx) results,
        equal to `cwt(...)` then `stx(...)` to within float rounding; `out` / `reduced_out` are pairs."""
        sig = self._signal(sig)
        n_ch = sig.shape[0]
        out = out or (None, None)
        reduced_out = reduced_out or (None, None)
        res_c, desc_c = self._outputs(_lib.QI_BANK_STYX, n_ch, coef, bits, reductions, power_scale, eps, out[0], reduced_out[0])
        res_s, desc_s = self._outputs(_lib.QI_TABLE_STX, n_ch, coef, bits, reductions, power_scale, eps, out[1], reduced_out[1])
        with torch.cuda.device(self.device):
            rc = self._lib.qi_cwt_stx(self._handle, _lib.QI_BANK_STYX, _lib.ptr(sig), n_ch, C.byref(desc_c),
                                      C.byref(desc_s), self._stream())
        _lib.check(rc)
        return res_c, res_s

    def cwt(self, sig, coef=True, bits=False, reductions=False, power_scale=1.0, eps=0.0, out=None, reduced_out=None):
        return self._run(_lib.QI_BANK_STYX, sig, coef, bits, reductions, power_scale, eps, out, reduced_out)

    def cwt_atoms(self, sig, coef=True, bits=False, reductions=False, power_scale=1.0, eps=0.0, out=None, reduced_out=None):
        return self._run(_lib.QI_BANK_ATOMS, sig, coef, bits, reductions, power_scale, eps, out, reduced_out)

    def stx(self, sig, coef=True, bits=False, reductions=False, power_scale=1.0, eps=0.0, out=None, reduced_out=None):
        return self._run(_lib.QI_TABLE_STX, sig, coef, bits, reductions, power_scale, eps, out, reduced_out)

    def _staged_panels(self, which, sig, power, power_scale, eps, tile_bytes):
        """The tile loop of pooled() and pooled_strip(): the records [C, n] go through transform `which` in tiles of
        max(1, tile_bytes // (B n element size)) records; each tile's panel (coefficients if `power`, else bits) lands in the
        staging tensor the plan keeps between calls (close() drops it).  Yields (first record, end record, panel
        [records, B, n]) after the tile's launches are queued; the panel is overwritten by the next tile."""
        f_hz = self.freq.get(which)
        if f_hz is None:
            raise _lib.QiError("band table not set on this plan")
        n_ch, n_b = sig.shape[0], len(f_hz)
        sdtype = _complex_of(self.rdtype) if power else self.rdtype
        per_record = n_b * self.n * torch.empty((), dtype=sdtype).element_size()
        tile = min(n_ch, max(1, int(tile_bytes) // per_record))
        if self._stage is None or self._stage.numel() < tile * per_record:
            self._stage = None  # (released before the larger one is made)
            self._stage = torch.empty(tile * per_record, dtype=torch.uint8, device=self.device)
        stage = self._stage[: tile * per_record].view(sdtype).view(tile, n_b, self.n)
        for c0 in range(0, n_ch, tile):
            c1 = min(n_ch, c0 + tile)
            panel = stage[: c1 - c0]
            res = TfrResult(frequency_hz=f_hz, coef=panel if power else None, bits=None if power else panel)
            self._run(which, sig[c0:c1], power, not power, False, power_scale, eps, out=res)
            yield c0, c1, panel

    def pooled(self, which, sig, factor, method="average", quantity="power", power_scale=1.0, eps=0.0, tile_bytes=1 << 30):
        """Transform `which` (QI_BANK_STYX, QI_BANK_ATOMS or QI_TABLE_STX) of records [C, n], pooled along time in windows of
        `factor` samples (utilities.sampling.subsample_2d's methods): -> device tensor [C, B, columns], real, in the plan's
        precision.  quantity "power": power_scale * |z|^2 of the coefficients; "bits": log2(|z| + eps).  The full panel never
        reaches the caller: the records go through in tiles of max(1, tile_bytes // (B n element size)) records, each tile's
        panel lands in a staging tensor the plan keeps between calls (close() drops it) and is pooled into its slice of the
        result by one kernel (qi_pool_panel) on the same stream.  Nothing is synchronised on the host."""
        from .utilities.sampling import _METHOD_CODE, pool_rows

        if quantity not in ("power", "bits"):
            raise ValueError(f'quantity must be "power" or "bits", got {quantity!r}')
        if method not in _METHOD_CODE:
            raise ValueError(f"method must be one of {sorted(_METHOD_CODE)}, got {method!r}")
        sig = self._signal(sig)
        f_hz = self.freq.get(which)
        if f_hz is None:
            raise _lib.QiError("band table not set on this plan")
        n_ch, n_b = sig.shape[0], len(f_hz)
        cols = int(self._lib.qi_pool_columns(self.n, int(factor), _METHOD_CODE[method]))
        if cols < 0:
            _lib.check(cols)
        power = quantity == "power"
        result = torch.empty((n_ch, n_b, cols), dtype=self.rdtype, device=self.device)
        for c0, c1, panel in self._staged_panels(which, sig, power, power_scale, eps, tile_bytes):
            pool_rows(panel, factor, method, _lib.QI_POOL_POWER if power else _lib.QI_POOL_REAL, power_scale, out=result[c0:c1])
        return result

    def pooled_strip(self, which, sig, factor, first, windows, methods=("average",), power_scale=1.0, tile_bytes=1 << 30):
        """The part of a pooled power panel that lies in the column range [first, first + windows factor) of transform `which`
        of records [C, n], and the additive reductions of that range -- what a streamed record keeps of the range a chunk
        owns (stream.owned_windows).  -> (strips, power_band, stats): strips {method: [C, B, windows]} in the plan's
        precision for methods out of ("average", "max"); power_band [C, B] float64, the sum of P = power_scale |z|^2 over
        the range; stats [C, 4] float64 = {max P, sum P, sum P log2 P, 0} over the range, as TfrResult.stats.  Tiles and
        staging tensor as pooled(); per tile one transform into the stage and ONE kernel (qi_pool_strip) that reads the range
        once for every output; the statistics are folded over the bands on the device (qi_pool_strip_stats).  Nothing is
        synchronised on the host."""
        methods = check_pooled_methods(methods, "methods")
        factor, first, windows = int(factor), int(first), int(windows)
        if factor < 2:
            raise ValueError(f"pooling factor {factor}: 2 or more")
        if first < 0 or windows < 0 or first + windows * factor > self.n:
            raise ValueError(f"{windows} windows of {factor} samples from sample {first} do not fit a record of {self.n}")
        sig = self._signal(sig)
        f_hz = self.freq.get(which)
        if f_hz is None:
            raise _lib.QiError("band table not set on this plan")
        n_ch, n_b = sig.shape[0], len(f_hz)
        strips = {m: torch.empty((n_ch, n_b, windows), dtype=self.rdtype, device=self.device) for m in methods}
        sums = torch.zeros((n_ch, n_b, 3), dtype=torch.float64, device=self.device)
        stats = torch.zeros((n_ch, 4), dtype=torch.float64, device=self.device)
        if windows == 0 or n_ch == 0:
            return strips, sums[:, :, 1].contiguous(), stats
        code = _lib.dtype_code(self.rdtype)
        mean, peak = strips.get("average"), strips.get("max")
        for c0, c1, panel in self._staged_panels(which, sig, True, power_scale, 0.0, tile_bytes):
            with torch.cuda.device(self.device):
                _lib.check(self._lib.qi_pool_strip(code, self.device.index, _lib.ptr(panel), (c1 - c0) * n_b, self.n, first, factor,
                                                   windows, float(power_scale), _lib.ptr(None if mean is None else mean[c0:c1]),
                                                   _lib.ptr(None if peak is None else peak[c0:c1]), windows, _lib.ptr(sums[c0:c1]),
                                                   self._stream()))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.qi_pool_strip_stats(self.device.index, _lib.ptr(sums), n_ch, n_b, _lib.ptr(stats), self._stream()))
        return strips, sums[:, :, 1].contiguous(), stats

    def close(self):
        self._stage = None
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.qi_plan_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanRing:
    """Independent records, one call each: `depth` plans with the same tables on `depth` streams, used in turn.

    A call of one or two records spends a fifth of its time in short launches (forward transform, coarse stage, tail) that
    leave most of the chip idle; inside ONE call they cannot be hidden (cross-stream events cost more than the overlap
    saves), between INDEPENDENT calls they can: the short launches of one call run under the long launches of the other
    (configs[1]: 434 000 against 387 000 Mpoints/s).  No cross-stream synchronisation happens here; every result carries
    the event that follows its launches.

        ring = PlanRing(n, torch.float32, setup=lambda p: (p.set_styx_bank(3, fs), p.set_stx_bands(3, fs)))
        for record in records:                       # [1, n] tensors on the device
            res_c, res_s, done = ring.cwt_stx(record, coef=True, reductions=True)
            ...                                      # done.synchronize() / stream.wait_event(done) before reading

    Results of a slot are overwritten `depth` calls later (they are the slot's `out=` buffers): consume or copy them
    before then.  `record` must not be modified before `done` either; it may be dropped (its memory is tied to the
    slot's stream with `record_stream`)."""

    def __init__(self, n, dtype=torch.float32, device=None, workspace_bytes=None, setup=None, depth=2,
                 engine=_lib.QI_ENGINE_AUTO, wait_input=True):
        self.wait_input = wait_input  # False: the caller guarantees the records are ready (no event on its stream)
        if depth < 1:
            raise ValueError("depth must be at least 1")
        self.plans = [TfrPlan(n, dtype, device, workspace_bytes, engine) for _ in range(depth)]
        for pl in self.plans:
            if setup is not None:
                setup(pl)
        self.streams = [torch.cuda.Stream(device=self.plans[0].device) for _ in range(depth)]
        self._outs = [dict() for _ in range(depth)]
        self._turn = 0

    def _call(self, name, sig, **kw):
        j = self._turn
        self._turn = (j + 1) % len(self.plans)
        stream = self.streams[j]
        if self.wait_input:  # the record was produced on the caller's stream
            stream.wait_stream(torch.cuda.current_stream(self.plans[j].device))
        key = (name, tuple(sig.shape), tuple(sorted(kw.items())))
        if sig.is_cuda:
            sig.record_stream(stream)  # the caller may drop the record: its memory is not reused before this stream is done
        with torch.cuda.stream(stream):
            res = getattr(self.plans[j], name)(sig, out=self._outs[j].get(key), **kw)
            self._outs[j][key] = res
            done = torch.cuda.Event()
            done.record(stream)
        return res, done

    def cwt_stx(self, sig, **kw):
        (res_c, res_s), done = self._call("cwt_stx", sig, **kw)
        return res_c, res_s, done

    def cwt(self, sig, **kw):
        return self._call("cwt", sig, **kw)

    def stx(self, sig, **kw):
        return self._call("stx", sig, **kw)

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def close(self):
        self.synchronize()
        for pl in self.plans:
            pl.close()
        self.plans = []


# ---- small LRU of plans for the reference-signature wrappers (each call there is one record) ----
# Safe from several host threads and streams.  A plan has one scratch (include/qi_tfr.h: one plan per host thread and stream at
# a time), so a caller BORROWS a plan and returns it behind its last launch: nobody else holds it meanwhile, and a plan in use
# is never closed.  A second concurrent caller of one key does not wait, it pays for a plan of its own.
_PLANS = collections.OrderedDict()  # the IDLE plans: serial -> _Idle, least recently returned first
_MAX_PLANS = 3
_PLANS_LOCK = threading.Lock()  # all bookkeeping; factory() and close() run outside it
_PLANS_SERIAL = 0
_PLANS_EPOCH = 0  # raised by clear_plans(): a plan borrowed in an earlier epoch is closed when it comes back

_Idle = collections.namedtuple("_Idle", "key plan done stream")  # done: event behind the last borrower's launches, on `stream`


def _close_idle(entries):
    for e in entries:
        if e.done is not None:
            e.done.synchronize()  # the last borrower's launches still use the scratch that close() frees
        e.plan.close()


@contextlib.contextmanager
def borrowed_plan(key, factory):
    """`with borrowed_plan(key, factory) as plan:` -- the idle plan of `key` returned last, or a new one from `factory()` when
    none is idle (another borrower holds it, or it was evicted).  Leave the block once the last launch that uses the plan has
    been queued: the cache then records an event on the current stream, and the next borrower's current stream waits for it on
    the device (nothing for the same stream; the host never waits).  Idle plans beyond _MAX_PLANS are closed, least recently
    returned first."""
    global _PLANS_SERIAL
    found = None
    with _PLANS_LOCK:
        epoch = _PLANS_EPOCH
        for serial in reversed(_PLANS):
            if _PLANS[serial].key == key:
                found = _PLANS.pop(serial)
                break
    if found is None:
        plan = factory()
    else:
        plan = found.plan
        if found.done is not None:
            stream = torch.cuda.current_stream(plan.device)
            if stream.cuda_stream != found.stream:
                stream.wait_event(found.done)
    try:
        yield plan
    finally:
        done = stream_id = None
        device = getattr(plan, "device", None)
        if device is not None:
            stream = torch.cuda.current_stream(device)
            if found is not None and found.done is not None and found.stream == stream.cuda_stream:
                done = found.done  # (the event is the plan's: recorded again, it stands for the later launches)
            else:
                done = torch.cuda.Event()
            done.record(stream)
            stream_id = stream.cuda_stream
        doomed = []
        with _PLANS_LOCK:
            if epoch != _PLANS_EPOCH:
                doomed.append(_Idle(key, plan, done, stream_id))
            else:
                _PLANS_SERIAL += 1
                _PLANS[_PLANS_SERIAL] = _Idle(key, plan, done, stream_id)
                while len(_PLANS) > _MAX_PLANS:
                    doomed.append(_PLANS.popitem(last=False)[1])
        _close_idle(doomed)


def clear_plans():
    """Close the idle plans; a plan that is borrowed now is closed when it comes back."""
    global _PLANS_EPOCH
    with _PLANS_LOCK:
        _PLANS_EPOCH += 1
        doomed = list(_PLANS.values())
        _PLANS.clear()
    _close_idle(doomed)


def gabor_atoms(n, p_re, p_im, omega, amp, device=None, x=None):
    """[B, n] complex128 device tensor of time-domain atoms (qi_gabor_atoms); x: the sample positions [n] (float64,
    in samples relative to the atom's centre) when they are not the centred uniform ones (qi_gabor_atoms_at)."""
    lib = _lib.require_gpu()
    dev = torch.device(device) if device is not None else default_device()
    keep = [_lib.darr(a) for a in (p_re, p_im, omega, amp)]
    out = torch.empty((len(keep[0][0]), n), dtype=torch.complex128, device=dev)
    if x is not None:
        if np.shape(x) != (n,):
            raise ValueError(f"x must hold the {n} sample positions of the atoms, got shape {np.shape(x)}")
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        with torch.cuda.device(dev):
            _lib.check(
                lib.qi_gabor_atoms_at(dev.index if dev.index is not None else torch.cuda.current_device(), n,
                                      len(keep[0][0]), keep[0][1], keep[1][1], keep[2][1], keep[3][1], _lib.ptr(xd),
                                      _lib.ptr(out), _lib.stream_ptr(dev))
            )
        return out
    with torch.cuda.device(dev):
        _lib.check(
            lib.qi_gabor_atoms(
                dev.index if dev.index is not None else torch.cuda.current_device(),
                n,
                len(keep[0][0]),
                keep[0][1],
                keep[1][1],
                keep[2][1],
                keep[3][1],
                _lib.ptr(out),
                _lib.stream_ptr(dev),
            )
        )
    return out


# ---- plan-less record calls: records [n] or [C, n] in, one library call on the current stream, `finish` out ----
def _matrix_stack(a, what, layout="[nf, C, C]", square=True):
    """A non-empty 3-d complex64 / complex128 stack, NumPy or tensor -> (contiguous device tensor, was_numpy, real dtype);
    square: its last two sides are equal (a stack of matrices)."""
    was_numpy = not isinstance(a, torch.Tensor)
    s = torch.from_numpy(np.ascontiguousarray(a)) if was_numpy else a
    if s.dim() != 3 or s.dtype not in (torch.complex64, torch.complex128) or 0 in s.shape or (square and s.shape[1] != s.shape[2]):
        raise ValueError(f"{what} must be a non-empty complex64 / complex128 {layout}, got {s.dtype} {tuple(s.shape)}")
    rdtype = torch.float32 if s.dtype == torch.complex64 else torch.float64
    return s.to(s.device if s.is_cuda else default_device()).contiguous(), was_numpy, rdtype


def cross_spectra(panel, weight=None, coherence=False):
    """Cross-spectra between the records of a stored coefficient panel [C, n_bands, n_time] (an STFT, CWT or Stockwell panel:
    complex64 or complex128): csd[f, i, j] = weight[f] sum_t conj(panel[i, f, t]) panel[j, f, t], one Hermitian matrix per
    band, summed on the matrix cores in the panel's precision (qi_cross_spectra).  weight: [n_bands] host values or None (1).
    -> csd [n_bands, C, C], or (csd, coherence [n_bands, C, C] = |S_ij|^2 / (S_ii S_jj)) with coherence=True.  NumPy in ->
    NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_f, n_t = z.shape
    w_host, w_ptr = (None, None)
    if weight is not None:
        w_host, w_ptr = _lib.darr(weight)
        if w_host.shape != (n_f,):
            raise ValueError(f"weight must hold one value per band ({n_f}), got shape {w_host.shape}")
    dev, code = z.device, _lib.dtype_code(rdtype)
    csd = torch.empty((n_f, n_ch, n_ch), dtype=z.dtype, device=dev)
    coh = torch.empty((n_f, n_ch, n_ch), dtype=rdtype, device=dev) if coherence else None
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_scratch_bytes, dev, code, n_ch, n_f, n_t)
    _lib.call(lib.qi_cross_spectra, dev, code, dev.index, _lib.ptr(z), n_ch, n_f, n_t, w_ptr, _lib.ptr(csd), _lib.ptr(coh),
              _lib.ptr(scratch), nbytes)
    if coherence:
        return finish(csd, was_numpy, False), finish(coh, was_numpy, False)
    return finish(csd, was_numpy, False)


def cross_spectra_windows(panel, window_segments, hop_segments=None, weight=None, bins=None, coherence=False):
    """cross_spectra per sliding window of the panel's time axis (qi_cross_spectra_windows): window w holds the columns
    w * hop_segments .. w * hop_segments + window_segments - 1 of panel [C, n_bands, n_time]; n_windows =
    (n_time - window_segments) // hop_segments + 1, columns after the last window are ignored.  hop_segments: None for
    max(1, window_segments // 2).  bins: (first, count) of the bands that are formed, or None (all).  weight: [count] host
    values, one per FORMED band, or None (1).  Window w equals cross_spectra(panel[:, first:first + count,
    w * hop:w * hop + window_segments], weight) bit for bit.
    -> csd [n_windows, count, C, C], or (csd, coherence [n_windows, count, C, C]) with coherence=True.  NumPy in -> NumPy out,
    CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_f, n_t = z.shape
    win = int(window_segments)
    hop = max(1, win // 2) if hop_segments is None else int(hop_segments)
    first, count = (0, n_f) if bins is None else (int(bins[0]), int(bins[1]))
    w_host, w_ptr = (None, None)
    if weight is not None:
        w_host, w_ptr = _lib.darr(weight)
        if w_host.shape != (count,):
            raise ValueError(f"weight must hold one value per formed band ({count}), got shape {w_host.shape}")
    dev, code = z.device, _lib.dtype_code(rdtype)
    # (the library refuses what is wrong with the windows and the bin range, before the outputs are shaped by them)
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_windows_scratch_bytes, dev, code, n_ch, n_f, n_t, first, count, win, hop)
    n_win = (n_t - win) // hop + 1
    csd = torch.empty((n_win, count, n_ch, n_ch), dtype=z.dtype, device=dev)
    coh = torch.empty((n_win, count, n_ch, n_ch), dtype=rdtype, device=dev) if coherence else None
    _lib.call(lib.qi_cross_spectra_windows, dev, code, dev.index, _lib.ptr(z), n_ch, n_f, n_t, first, count, win, hop, w_ptr,
              _lib.ptr(csd), _lib.ptr(coh), _lib.ptr(scratch), nbytes)
    if coherence:
        return finish(csd, was_numpy, False), finish(coh, was_numpy, False)
    return finish(csd, was_numpy, False)


def cross_spectra_bands(panel, terms, hop=None, stride=None, weight=None, bins=None, coherence=False):
    """cross_spectra of a constant-Q panel [C, n_bands, n_time] (a CWT or Stockwell panel), every formed band in a window, hop
    and sample stride of its own (qi_cross_spectra_bands, include/qi_bands.h): window w of band b sums the columns
    w * hop[b] + k * stride[b], k = 0 .. terms[b] - 1; span[b] = (terms[b] - 1) * stride[b] + 1, n_windows[b] =
    (n_time - span[b]) // hop[b] + 1, columns after a band's last window are ignored.  bins: (first, count) of the bands that
    are formed, or None (all).  terms, hop, stride: [count] host integers, one per FORMED band; stride None: 1; hop None:
    max(1, span // 2).  weight: [count] host values or None (1).  The matrices of all bands come from one launch as a ragged,
    band-major stack: band b's windows are the rows offsets[b] .. offsets[b + 1] - 1, and row offsets[b] + w equals
    cross_spectra(panel[:, first + b:first + b + 1, w * hop[b]:w * hop[b] + span[b]:stride[b]], weight[b:b + 1]) bit for bit.
    -> (offsets [count + 1] np.int64, csd [total, C, C]), or (offsets, csd, coherence [total, C, C]) with coherence=True.
    NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_b, n_t = z.shape
    first, count = (0, n_b) if bins is None else (int(bins[0]), int(bins[1]))
    if count < 1:
        raise ValueError(f"bins must hold at least one band, got {bins}")

    def table(a, what):
        host, p = _lib.iarr(a)
        if host.shape != (count,):
            raise ValueError(f"{what} must hold one value per formed band ({count}), got shape {host.shape}")
        return host, p

    t_host, t_ptr = table(terms, "terms")
    s_host, s_ptr = table(np.ones(count, dtype=np.int64) if stride is None else stride, "stride")
    h_host, h_ptr = table(np.maximum(1, ((t_host - 1) * s_host + 1) // 2) if hop is None else hop, "hop")
    w_host, w_ptr = (None, None)
    if weight is not None:
        w_host, w_ptr = _lib.darr(weight)
        if w_host.shape != (count,):
            raise ValueError(f"weight must hold one value per formed band ({count}), got shape {w_host.shape}")
    dev, code = z.device, _lib.dtype_code(rdtype)
    # (the library refuses what is wrong with the tables and the band range, before the outputs are shaped by them)
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_bands_scratch_bytes, dev, code, n_ch, n_b, n_t, first, count, t_ptr, h_ptr, s_ptr)
    offsets = np.empty(count + 1, dtype=np.int64)
    total = int(lib.qi_cross_spectra_bands_layout(n_t, count, t_ptr, h_ptr, s_ptr, offsets.ctypes.data_as(_lib._I64)))
    csd = torch.empty((total, n_ch, n_ch), dtype=z.dtype, device=dev)
    coh = torch.empty((total, n_ch, n_ch), dtype=rdtype, device=dev) if coherence else None
    _lib.call(lib.qi_cross_spectra_bands, dev, code, dev.index, _lib.ptr(z), n_ch, n_b, n_t, first, count, t_ptr, h_ptr, s_ptr, w_ptr,
              _lib.ptr(csd), _lib.ptr(coh), _lib.ptr(scratch), nbytes)
    if coherence:
        return offsets, finish(csd, was_numpy, False), finish(coh, was_numpy, False)
    return offsets, finish(csd, was_numpy, False)


def _band_table(values, count, what):
    """A host table of one float64 per band, or None -> (array kept alive, pointer for the library)."""
    if values is None:
        return None, None
    host, p = _lib.darr(values)
    if host.shape != (count,):
        raise ValueError(f"{what} must hold one value per band ({count}), got shape {host.shape}")
    return host, p


def _bin_edges(edges_hz):
    host, p = _lib.darr(edges_hz)
    if host.ndim != 1 or len(host) < 2:
        raise ValueError(f"edges_hz must hold the edges of one bin at least, got shape {host.shape}")
    return host, p, len(host) - 1


def instantaneous_frequency(panel, sample_rate_hz, carrier_hz=None, power_floor=0.0):
    """The instantaneous frequency in Hz of every coefficient of a panel [C, n_bands, n_time] (a CWT or Stockwell panel,
    complex64 or complex128), from the forward phase difference along time (qi_tfr_ifreq, include/qi_squeeze.h):
    carrier_hz[b] + sample_rate_hz * angle(panel[.., t + 1] * conj(panel[.., t])) / (2 pi); the last column takes the
    difference behind it.  carrier_hz: [n_bands] host values or None (0) -- the frequency band b has been demodulated by: 0
    for a CWT panel, the snapped bin frequency stx_shift_indices * sample_rate_hz / n for a Stockwell panel.  An element is
    NaN where |coefficient|^2 of it or of its partner is below power_floor or not finite.  -> [C, n_bands, n_time] real.
    NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_b, n_t = z.shape
    c_host, c_ptr = _band_table(carrier_hz, n_b, "carrier_hz")
    dev, code = z.device, _lib.dtype_code(rdtype)
    scratch, nbytes = _lib.scratch(lib.qi_tfr_squeeze_scratch_bytes, dev, code, n_ch, n_b, n_t, 1)
    out = torch.empty((n_ch, n_b, n_t), dtype=rdtype, device=dev)
    _lib.call(lib.qi_tfr_ifreq, dev, code, dev.index, _lib.ptr(z), n_ch, n_b, n_t, c_ptr, float(sample_rate_hz), float(power_floor),
              _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, False)


def squeeze(panel, ifreq, edges_hz, weight=None):
    """Reassignment of a panel [C, n_bands, n_time] to frequency bins by the frequencies it is handed (qi_tfr_squeeze):
    out[c, k, t] = sum of weight[b] * panel[c, b, t] over the bands with edges_hz[k] <= ifreq[c, b, t] < edges_hz[k + 1], added
    in ascending b in the panel's precision.  ifreq: [C, n_bands, n_time] real of the panel's precision (NaN: the element is
    dropped); edges_hz: [n_bins + 1] strictly ascending host values; weight: [n_bands] host values or None (1).  The result
    is exact given the frequencies, the same bits in every run: no atomics.  -> [C, n_bins, n_time] complex.  NumPy in ->
    NumPy out, CUDA tensor in -> CUDA tensor out (the panel decides)."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_b, n_t = z.shape
    f = torch.from_numpy(np.ascontiguousarray(ifreq)) if not isinstance(ifreq, torch.Tensor) else ifreq
    if f.dtype != rdtype or tuple(f.shape) != tuple(z.shape):
        raise ValueError(f"ifreq must be {rdtype} {tuple(z.shape)}, got {f.dtype} {tuple(f.shape)}")
    f = f.to(z.device).contiguous()
    e_host, e_ptr, n_bins = _bin_edges(edges_hz)
    w_host, w_ptr = _band_table(weight, n_b, "weight")
    dev, code = z.device, _lib.dtype_code(rdtype)
    scratch, nbytes = _lib.scratch(lib.qi_tfr_squeeze_scratch_bytes, dev, code, n_ch, n_b, n_t, n_bins)
    out = torch.empty((n_ch, n_bins, n_t), dtype=z.dtype, device=dev)
    _lib.call(lib.qi_tfr_squeeze, dev, code, dev.index, _lib.ptr(z), _lib.ptr(f), n_ch, n_b, n_t, e_ptr, n_bins, w_ptr, _lib.ptr(out),
              _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, False)


def synchrosqueeze(panel, sample_rate_hz, edges_hz, carrier_hz=None, weight=None, power_floor=0.0):
    """The synchrosqueezed panel in one pass (qi_tfr_synchrosqueeze): squeeze(panel, instantaneous_frequency(panel,
    sample_rate_hz, carrier_hz, power_floor), edges_hz, weight) bit for bit, without the frequencies ever reaching device
    memory.  -> [C, n_bins, n_time] complex.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_b, n_t = z.shape
    c_host, c_ptr = _band_table(carrier_hz, n_b, "carrier_hz")
    w_host, w_ptr = _band_table(weight, n_b, "weight")
    e_host, e_ptr, n_bins = _bin_edges(edges_hz)
    dev, code = z.device, _lib.dtype_code(rdtype)
    scratch, nbytes = _lib.scratch(lib.qi_tfr_squeeze_scratch_bytes, dev, code, n_ch, n_b, n_t, n_bins)
    out = torch.empty((n_ch, n_bins, n_t), dtype=z.dtype, device=dev)
    _lib.call(lib.qi_tfr_synchrosqueeze, dev, code, dev.index, _lib.ptr(z), n_ch, n_b, n_t, c_ptr, float(sample_rate_hz),
              float(power_floor), e_ptr, n_bins, w_ptr, _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, False)


def pair_lags(csd, *, bins=None, weighting="phat", halve_interior=True, normalize=True, upsample=1, max_lag=None, want_cc=False):
    """Time delays between every pair of records from their cross-spectral matrices (qi_pair_lags, include/qi_lags.h): the
    generalized cross-correlation r of pair (i, j), i < j, its first maximum inside +-max_lag and the three-point parabola
    through it, in one launch.  csd: [nf, C, C] complex64 / complex128 as cross_spectra and styx_fft.csd_matrix_pow2 return
    it, or a stack [nstack, nf, C, C] (cross_spectra_windows / styx_fft.csd_windows_pow2 with every bin); nf = nfft / 2 + 1
    with nfft a power of two, nfft * upsample in 64 .. 8192.  bins: (lo, hi) -- the bins lo <= f < hi enter, the rest count
    as 0 -- or None (all).  weighting: "plain", "phat" (1 / |S_ij|) or "scot" (1 / sqrt(S_ii S_jj)).  halve_interior: halve
    the bins 0 < f < nfft / 2 (undoes the one-sided doubling of csd_matrix_pow2).  normalize: plain -> the correlation
    coefficient; phat / scot -> divided by the count of non-zero two-sided bins, a peak of at most 1.  upsample: 1, 2, 4 or 8,
    the zero padding of the spectrum -- lags of the window and max_lag are in samples of that finer grid.  max_lag: None for
    the largest, nfft * upsample / 2 - 1.  With csd[f, i, j] = conj(X_i) X_j a positive lag means record j lags record i.
    -> (peak_lag [npair] in samples of the RECORDS, peak_value [npair], cc [npair, 2 max_lag + 1] or None), npair =
    C (C - 1) / 2 in the order (0, 1), (0, 2) .. (C - 2, C - 1), with the leading stack dimension when csd has one.  A pair
    whose band holds a non-finite entry is NaN.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    was_numpy = not isinstance(csd, torch.Tensor)
    s = torch.from_numpy(np.ascontiguousarray(csd)) if was_numpy else csd
    if s.dim() not in (3, 4) or s.dtype not in (torch.complex64, torch.complex128) or 0 in s.shape or s.shape[-1] != s.shape[-2]:
        raise ValueError(f"csd must be a non-empty complex64 / complex128 [nf, C, C] or [nstack, nf, C, C], got {s.dtype} {tuple(s.shape)}")
    stacked = s.dim() == 4
    s = s.to(s.device if s.is_cuda else default_device()).contiguous()
    rdtype = torch.float32 if s.dtype == torch.complex64 else torch.float64
    n_stack = s.shape[0] if stacked else 1
    n_f, n_ch = s.shape[-3], s.shape[-1]
    nfft = 2 * (n_f - 1)
    if weighting not in _lib.LAG_WEIGHTINGS:
        raise ValueError(f"weighting must be one of {_lib.LAG_WEIGHTINGS}, got {weighting!r}")
    lo, hi = (0, n_f) if bins is None else (int(bins[0]), int(bins[1]))
    up = int(upsample)
    dev, code = s.device, _lib.dtype_code(rdtype)
    # (the library refuses what is wrong with the shape, before the outputs are shaped by it)
    scratch, nbytes = _lib.scratch(lib.qi_pair_lags_scratch_bytes, dev, code, n_stack, n_ch, nfft, up)
    lag = nfft * up // 2 - 1 if max_lag is None else int(max_lag)
    n_pair = n_ch * (n_ch - 1) // 2
    peak_lag = torch.empty((n_stack, n_pair), dtype=rdtype, device=dev)
    peak_value = torch.empty((n_stack, n_pair), dtype=rdtype, device=dev)
    cc = torch.empty((n_stack, n_pair, 2 * max(lag, 0) + 1), dtype=rdtype, device=dev) if want_cc else None
    _lib.call(lib.qi_pair_lags, dev, code, dev.index, _lib.ptr(s), n_stack, n_ch, nfft, lo, hi, _lib.LAG_WEIGHTINGS.index(weighting),
              int(bool(halve_interior)), int(bool(normalize)), up, lag, _lib.ptr(cc), _lib.ptr(peak_lag), _lib.ptr(peak_value),
              _lib.ptr(scratch), nbytes)
    return tuple(finish(t, was_numpy, not stacked) for t in (peak_lag, peak_value, cc))


def delay_bank(phases=64, taps=8, beta=5.0, dtype=torch.float32):
    """The polyphase fractional-delay bank of time_beam_power and time_beam_traces: row p of [phases, taps] interpolates a
    record at the fraction p / phases of a sample past the tap c = (taps - 1) // 2 -- a Kaiser-windowed sinc.  With
    k = m - c, u = k - p / P and a = u / (T / 2): h = sinc(u) I0(beta sqrt(1 - a^2)) / I0(beta) for |a| <= 1, else 0; every row
    is divided by its sum (unit gain at 0 Hz).  Row 0 is the exact unit impulse at m = c; taps = 1 requires phases = 1 and is
    [[1]] (whole-sample delays).  Built on the host in float64 with NumPy alone, then rounded to `dtype`.
    -> [phases, taps] tensor of float32 or float64 on the host (the calls take it to the records' device)."""
    p_count, t_count = int(phases), int(taps)
    if t_count not in _lib.TIMEBEAM_TAPS or not 1 <= p_count <= _lib.TIMEBEAM_MAX_PHASES:
        raise ValueError(f"delay_bank takes taps of {_lib.TIMEBEAM_TAPS} and 1 .. {_lib.TIMEBEAM_MAX_PHASES} phases, got {taps} and {phases}")
    if t_count == 1 and p_count != 1:
        raise ValueError("a bank of one tap delays by whole samples: it has one phase")
    rdtype = _real_dtype(dtype)
    centre = (t_count - 1) // 2
    k = (np.arange(t_count) - centre).astype(np.float64)[None, :]
    u = k - (np.arange(p_count).astype(np.float64) / p_count)[:, None]
    a = u / (t_count / 2.0)
    inside = np.abs(a) <= 1.0
    h = np.where(inside, np.sinc(u) * np.i0(float(beta) * np.sqrt(np.where(inside, 1.0 - a * a, 0.0))) / np.i0(float(beta)), 0.0)
    h = h / h.sum(axis=1, keepdims=True)
    h[0] = 0.0
    h[0, centre] = 1.0
    return torch.from_numpy(np.ascontiguousarray(h)).to(rdtype)


def quantize_delays(delays_s, sample_rate_hz, phases, device=None):
    """Delays in seconds [rows, C] (NumPy or tensor; plane_wave_delays' result) as whole samples and bank phases:
    q = floor(tau rate P + 0.5), shift = q // P, phase = q mod P (floor division: 0 <= phase < P for negative delays too).
    The beam of time_beam_power / time_beam_traces aligns with x_i[t + tau_i]: a plane wave that reaches sensor i later by
    tau_i = plane_wave_delays(...) adds coherently at its own slowness, the sign convention of beamform.
    -> (shift [rows, C] int32, phase [rows, C] int32, both on the device; max_shift: the largest |shift|, a Python int)."""
    tau = delays_s.detach().cpu().to(torch.float64).numpy() if isinstance(delays_s, torch.Tensor) else np.asarray(delays_s, dtype=np.float64)
    p_count = int(phases)
    if tau.ndim != 2 or tau.size == 0 or not np.isfinite(tau).all() or p_count < 1:
        raise ValueError(f"delays_s must be a finite non-empty [rows, C] and phases positive, got shape {tuple(tau.shape)} and {phases}")
    q = np.floor(tau * float(sample_rate_hz) * p_count + 0.5)
    shift = np.floor_divide(q, p_count)
    phase = q - shift * p_count
    if np.abs(shift).max() >= 2.0 ** 31:
        raise ValueError("a delay of more than 2^31 samples")
    if device is None:
        device = delays_s.device if isinstance(delays_s, torch.Tensor) and delays_s.is_cuda else default_device()
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(device)  # noqa: E731
    return to_dev(shift), to_dev(phase), int(np.abs(shift).max())


def _time_beam_inputs(sig, shift, phase, bank, max_shift):
    """What time_beam_power and time_beam_traces share -> (records [C, n] on the device, was_numpy, shift, phase, bank on
    that device and contiguous, rows, phases, taps, max_shift)."""
    x, was_numpy, _ = as_signal(sig)
    x = x.contiguous()
    dev = x.device
    tables = []
    for name, t in (("shift", shift), ("phase", phase)):
        t = torch.from_numpy(np.ascontiguousarray(t)) if not isinstance(t, torch.Tensor) else t
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != x.shape[0] or t.dtype.is_floating_point or t.dtype.is_complex:
            raise ValueError(f"{name} must be whole numbers [rows, {x.shape[0]}], got {t.dtype} {tuple(t.shape)}")
        tables.append(t.to(dev).to(torch.int32).contiguous())
    if tables[0].shape != tables[1].shape:
        raise ValueError(f"shift {tuple(tables[0].shape)} and phase {tuple(tables[1].shape)} differ in shape")
    h = torch.from_numpy(np.ascontiguousarray(bank)) if not isinstance(bank, torch.Tensor) else bank
    if h.dim() != 2 or 0 in h.shape:
        raise ValueError(f"bank must be [phases, taps], got shape {tuple(h.shape)}")
    h = h.to(dev).to(x.dtype).contiguous()
    return x, was_numpy, tables[0], tables[1], h, tables[0].shape[0], h.shape[0], h.shape[1], int(max_shift)


def time_beam_power(sig, shift, phase, bank, window_points, hop_points, max_shift, normalize=True, peaks=True):
    """Delay-and-sum power of the records of an array per sliding window and delay row, in the time domain
    (qi_time_beam_power, include/qi_timebeam.h): y[g, i, t] = sum_m bank[phase[g, i], m] x[i, t + shift[g, i] + m - c],
    c = (taps - 1) // 2, x zero outside the record; b = sum_i y; over the window t in [w hop, w hop + win):
    normalize=False -> sum b^2 / (C^2 win), the mean square of the beam; normalize=True -> sum b^2 / (C sum_i sum y^2), the
    semblance in [0, 1] (NaN where the delayed records are all zero).  sig: [C, n] float32 / float64, 2 <= C <= 64; shift,
    phase: [G, C] whole numbers (quantize_delays); bank: [P, T] (delay_bank); max_shift: the largest |shift| the call has
    to take -- a row beyond it, or with a phase outside 0 .. P - 1, is NaN.  Any delay length: up to max_shift = 1024 the
    records are staged in LDS, beyond that the same arithmetic reads through L2 (the same bits, slower).
    -> power [nwin, G], or (power, peak_index [nwin] int64, peak_value [nwin]) with peaks=True: np.argmax of every window's
    row and that entry.  nwin = 1 + (n - win) // hop.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    x, was_numpy, sh, ph, h, n_rows, n_phase, n_taps, reach = _time_beam_inputs(sig, shift, phase, bank, max_shift)
    n_ch, n = x.shape
    win, hop = int(window_points), int(hop_points)
    dev, code = x.device, _lib.dtype_code(x.dtype)
    # (the library refuses what is wrong with the shape, before the outputs are shaped by it)
    scratch, nbytes = _lib.scratch(lib.qi_time_beam_power_scratch_bytes, dev, code, n_ch, n, n_phase, n_taps, n_rows, win, hop, reach)
    n_win = 1 + (n - win) // hop
    power = torch.empty((n_win, n_rows), dtype=x.dtype, device=dev)
    index = torch.empty(n_win, dtype=torch.int64, device=dev) if peaks else None
    value = torch.empty(n_win, dtype=x.dtype, device=dev) if peaks else None
    _lib.call(lib.qi_time_beam_power, dev, code, dev.index, _lib.ptr(x), n_ch, n, _lib.ptr(h), n_phase, n_taps, _lib.ptr(sh), _lib.ptr(ph),
              n_rows, reach, win, hop, int(bool(normalize)), _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)
    if not peaks:
        return finish(power, was_numpy, False)
    return tuple(finish(t, was_numpy, False) for t in (power, index, value))


def time_beam_traces(sig, shift, phase, bank, max_shift):
    """Delay-and-sum beam traces of the records of an array (qi_time_beam_traces, include/qi_timebeam.h): traces[k, t] =
    (1 / C) sum_i sum_m bank[phase[k, i], m] x[i, t + shift[k, i] + m - c] for every sample of the record, x zero outside
    it; the arguments are time_beam_power's.  One launch; no [K, C, n] intermediate exists.  Zero delays and the impulse
    bank give the mean of the records.  -> traces [K, n].  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    x, was_numpy, sh, ph, h, n_rows, n_phase, n_taps, reach = _time_beam_inputs(sig, shift, phase, bank, max_shift)
    n_ch, n = x.shape
    dev, code = x.device, _lib.dtype_code(x.dtype)
    out = torch.empty((n_rows, n), dtype=x.dtype, device=dev)
    _lib.call(lib.qi_time_beam_traces, dev, code, dev.index, _lib.ptr(x), n_ch, n, _lib.ptr(h), n_phase, n_taps, _lib.ptr(sh), _lib.ptr(ph),
              n_rows, reach, _lib.ptr(out))
    return finish(out, was_numpy, False)


def _delay_grid_form(name, matrices, what, frequency_hz, delays_s, bands, peaks, *form_args, form_first=()):
    """What beam_power, capon_power and music_power share: the checks of the stack `what`, of frequency_hz, delays_s and bands,
    the scratch of qi_<name>_scratch_bytes, the outputs, the call of qi_<name> (form_first: what it takes between nf and
    freq_hz; form_args: between nb and power) and finish."""
    lib = _lib.require_gpu()
    s, was_numpy, rdtype = _matrix_stack(matrices, what)
    n_f, n_ch, _ = s.shape
    dev = s.device
    f_host, f_ptr = _lib.darr(frequency_hz)
    if f_host.shape != (n_f,):
        raise ValueError(f"frequency_hz must hold one value per matrix ({n_f}), got shape {f_host.shape}")
    tau = delays_s if isinstance(delays_s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(delays_s))
    if tau.dim() != 2 or tau.shape[0] < 1 or tau.shape[1] != n_ch:
        raise ValueError(f"delays_s must be [G, {n_ch}], got shape {tuple(tau.shape)}")
    tau = tau.to(dev).to(torch.float64).contiguous()
    n_g = tau.shape[0]
    b_host, b_ptr = (None, None) if bands is None else _lib.iarr(bands)
    if b_host is not None and (b_host.ndim != 1 or b_host.size < 2):
        raise ValueError(f"bands must be a list of nb + 1 offsets, got shape {b_host.shape}")
    n_b = n_f if b_host is None else b_host.size - 1
    code = _lib.dtype_code(rdtype)
    scratch, nbytes = _lib.scratch(getattr(lib, f"qi_{name}_scratch_bytes"), dev, code, n_ch, n_f, n_g, n_b)
    power = torch.empty((n_b, n_g), dtype=rdtype, device=dev)
    index = torch.empty(n_b, dtype=torch.int64, device=dev) if peaks else None
    value = torch.empty(n_b, dtype=rdtype, device=dev) if peaks else None
    _lib.call(getattr(lib, f"qi_{name}"), dev, code, dev.index, _lib.ptr(s), n_ch, n_f, *form_first, f_ptr, _lib.ptr(tau), n_g, b_ptr,
              n_b, *form_args, _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)
    if peaks:
        return finish(power, was_numpy, False), finish(index, was_numpy, False), finish(value, was_numpy, False)
    return finish(power, was_numpy, False)


def beam_power(csd, frequency_hz, delays_s, bands=None, normalize=False, peaks=False):
    """Steered (Bartlett) power of cross-spectral matrices over a grid of delay sets (qi_beam_power): with
    e[f, g, i] = exp(2 pi i frequency_hz[f] delays_s[g, i]), Q[f, g] = Re sum_ij conj(e_i) csd[f, i, j] e_j, summed over the
    matrices of each band and divided by C^2 -- or, normalize=True, by C sum_f trace(csd[f]): the semblance.
    csd: [nf, C, C] complex64 / complex128 as cross_spectra and styx_fft.csd_matrix_pow2 return it, C <= 64;
    frequency_hz: [nf] host values; delays_s: [G, C] seconds, NumPy or tensor, converted to float64 on the device (the
    phase is formed in double whatever the matrices' precision); bands: nb + 1 strictly ascending offsets into 0..nf or None
    (every matrix its own band).  -> power [nb, G] real, or (power, peak_index [nb] int64, peak_value [nb]) with peaks=True:
    np.argmax of every band's row and that entry.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    return _delay_grid_form("beam_power", csd, "csd", frequency_hz, delays_s, bands, peaks, int(bool(normalize)))


def csd_whiten(csd, loading=0.0, info=False):
    """Whitening factors of Hermitian cross-spectral matrices (qi_csd_whiten), what capon_power consumes: for every matrix
    R = csd[f] + loading * mean(diag csd[f]) I = L L^H (Cholesky), whitener[f] = V = L^-H -- upper triangular, R^-1 = V V^H,
    V^H R V = I.  csd: [nf, C, C] complex64 / complex128 as cross_spectra and styx_fft.csd_matrix_pow2 return it, C <= 64;
    only the lower triangle and the real part of the diagonal are read.  loading >= 0, relative to the mean auto-power.
    -> whitener [nf, C, C], or (whitener, info [nf] int32) with info=True: 0, or the 1-based index of the first pivot that is
    not a positive finite number (LAPACK's potrf); such a matrix's whitener is NaN on and above the diagonal.  NumPy in ->
    NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    s, was_numpy, rdtype = _matrix_stack(csd, "csd")
    n_f, n_ch, _ = s.shape
    dev = s.device
    code = _lib.dtype_code(rdtype)
    whitener = torch.empty_like(s)
    flags = torch.empty(n_f, dtype=torch.int32, device=dev) if info else None
    _lib.call(lib.qi_csd_whiten, dev, code, dev.index, _lib.ptr(s), n_ch, n_f, float(loading), _lib.ptr(whitener), _lib.ptr(flags))
    if info:
        return finish(whitener, was_numpy, False), finish(flags, was_numpy, False)
    return finish(whitener, was_numpy, False)


def capon_power(whitener, frequency_hz, delays_s, bands=None, peaks=False):
    """Capon (minimum-variance) power of whitened cross-spectral matrices over a grid of delay sets (qi_beam_capon): with
    e[f, g, i] = exp(2 pi i frequency_hz[f] delays_s[g, i]) and V = whitener[f], D[f, g] = sum_j |sum_i conj(V[i, j]) e_i|^2
    = e^H R^-1 e, and power[b, g] = sum over the band's matrices of 1 / D -- in the units of beam_power with normalize=False,
    and never above it on the same loaded matrices.  whitener: [nf, C, C] complex64 / complex128 as csd_whiten returns it,
    C <= 64; frequency_hz, delays_s, bands and peaks: as in beam_power.  A band that holds a matrix csd_whiten flagged is NaN,
    and its peak the first NaN.  -> power [nb, G] real, or (power, peak_index [nb] int64, peak_value [nb]) with peaks=True.
    NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    return _delay_grid_form("beam_capon", whitener, "whitener", frequency_hz, delays_s, bands, peaks)


def csd_eigh(csd, info=False):
    """Eigenpairs of Hermitian cross-spectral matrices (qi_csd_eigh), what music_power consumes: for every matrix
    csd[f] = U diag(w) U^H with w ascending and U^H U = I -- numpy.linalg.eigh's layout, column j of U the unit eigenvector of
    w[j]; the phase of a column is the iteration's, a function of the matrix alone.  csd: [nf, C, C] complex64 / complex128 as
    cross_spectra and styx_fft.csd_matrix_pow2 return it, C <= 64; only the lower triangle and the real part of the diagonal
    are read.  -> (eigenvalues [nf, C] real, eigenvectors [nf, C, C]), or (eigenvalues, eigenvectors, info [nf] int32) with
    info=True: 0, or 1 for a matrix that did not converge within the sweep cap -- every matrix with an entry that is not finite
    does not; such a matrix's eigenvalues and eigenvectors are NaN.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    s, was_numpy, rdtype = _matrix_stack(csd, "csd")
    n_f, n_ch, _ = s.shape
    dev = s.device
    code = _lib.dtype_code(rdtype)
    values = torch.empty((n_f, n_ch), dtype=rdtype, device=dev)
    vectors = torch.empty_like(s)
    flags = torch.empty(n_f, dtype=torch.int32, device=dev) if info else None
    _lib.call(lib.qi_csd_eigh, dev, code, dev.index, _lib.ptr(s), n_ch, n_f, _lib.ptr(values), _lib.ptr(vectors), _lib.ptr(flags))
    out = (finish(values, was_numpy, False), finish(vectors, was_numpy, False))
    return out + (finish(flags, was_numpy, False),) if info else out


def music_power(eigenvectors, n_sources, frequency_hz, delays_s, bands=None, peaks=False):
    """MUSIC power of diagonalised cross-spectral matrices over a grid of delay sets (qi_beam_music): with
    e[f, g, i] = exp(2 pi i frequency_hz[f] delays_s[g, i]), U = eigenvectors[f] and m = C - n_sources noise columns,
    D[f, g] = sum_{j < m} |sum_i conj(U[i, j]) e_i|^2 = e^H P_noise e, and power[b, g] = C n_b / (sum of D over the band's n_b
    matrices): the reciprocal of the band's mean null spectrum, dimensionless, >= 1 up to rounding and large at a source.
    eigenvectors: [nf, C, C] complex64 / complex128 as csd_eigh returns it, C <= 64; n_sources: 0 <= n_sources < C, one number
    for all matrices; frequency_hz, delays_s, bands and peaks: as in beam_power.  A band that holds a matrix csd_eigh flagged
    is NaN, and its peak the first NaN.  -> power [nb, G] real, or (power, peak_index [nb] int64, peak_value [nb]) with
    peaks=True.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    n = int(n_sources)
    if n != n_sources:
        raise ValueError(f"n_sources must be a whole number, got {n_sources!r}")
    return _delay_grid_form("beam_music", eigenvectors, "eigenvectors", frequency_hz, delays_s, bands, peaks, form_first=(n,))


def beam_weights(frequency_hz, delays_s, whitener=None, sensors=None, dtype=None):
    """Beam weights of nf bins over nbeam delay rows (qi_beam_weights), what beam_steer applies: with
    e[f, k, i] = exp(2 pi i frequency_hz[f] delays_s[k, i]), the conventional (Bartlett, delay-and-sum) weights a = e / C, or,
    with the whiteners V of csd_whiten (R^-1 = V V^H), the minimum-variance distortionless-response (MVDR) weights
    u = V^H e, D = sum_j |u_j|^2, a = V u / D = R^-1 e / (e^H R^-1 e): the a that minimises a^H R a under e^H a = 1, with
    a^H R a = 1 / D, the power capon_power gives.  frequency_hz: [nf] host values; delays_s: [nbeam, C] seconds, NumPy or
    tensor, converted to float64 on the device; whitener: [nf, C, C] complex64 / complex128 or None.  With a whitener C and the
    precision are its own; without one C is delays_s.shape[1] (sensors, if given, must agree) and dtype float32 (the default) or
    float64.  A bin whose whitener csd_whiten flagged has NaN weights.  -> weights [nf, nbeam, C] complex.  NumPy in (the
    whitener, or the delays without one) -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    f_host, f_ptr = _lib.darr(frequency_hz)
    if f_host.ndim != 1 or f_host.size < 1:
        raise ValueError(f"frequency_hz must be a non-empty list of bin frequencies, got shape {f_host.shape}")
    tau = delays_s if isinstance(delays_s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(delays_s))
    if whitener is not None:
        v, was_numpy, rdtype = _matrix_stack(whitener, "whitener")
        if dtype is not None and _real_dtype(dtype) != rdtype:
            raise ValueError(f"dtype {dtype} given with a {v.dtype} whitener: the precision is the whitener's")
        n_f, n_ch, dev = v.shape[0], v.shape[1], v.device
        if f_host.shape != (n_f,):
            raise ValueError(f"frequency_hz must hold one value per matrix ({n_f}), got shape {f_host.shape}")
    else:
        v, was_numpy = None, not isinstance(delays_s, torch.Tensor)
        rdtype = torch.float32 if dtype is None else _real_dtype(dtype)
        if rdtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be float32 or float64, got {dtype}")
        n_f, n_ch = f_host.size, (tau.shape[1] if tau.dim() == 2 else -1)
        dev = tau.device if tau.is_cuda else default_device()
    if sensors is not None and int(sensors) != n_ch:
        raise ValueError(f"sensors={sensors}, but the {'whitener' if v is not None else 'delays'} hold {n_ch}")
    if tau.dim() != 2 or tau.shape[0] < 1 or tau.shape[1] != n_ch:
        raise ValueError(f"delays_s must be [nbeam, {n_ch if n_ch > 0 else 'C'}], got shape {tuple(tau.shape)}")
    tau = tau.to(dev).to(torch.float64).contiguous()
    n_k = tau.shape[0]
    code = _lib.dtype_code(rdtype)
    scratch, nbytes = _lib.scratch(lib.qi_beam_weights_scratch_bytes, dev, code, n_ch, n_f, n_k)
    weights = torch.empty((n_f, n_k, n_ch), dtype=_complex_of(rdtype), device=dev)
    _lib.call(lib.qi_beam_weights, dev, code, dev.index, _lib.ptr(v), n_ch, n_f, f_ptr, _lib.ptr(tau), n_k, _lib.ptr(weights),
              _lib.ptr(scratch), nbytes)
    return finish(weights, was_numpy, False)


def beam_steer(panel, weights):
    """Beams of a stored coefficient panel (qi_beam_steer): out[k, f, t] = sum_i weights[f, k, i] panel[i, f, t], summed on the
    matrix cores in the panel's precision.  There is no conjugate: with cross_spectra's csd = conj(Z_i) Z_j,
    mean_t |out|^2 = a^H csd a, and beam_weights' a = e / C aligns a plane wave that reaches sensor i later by delays_s[k, i].
    panel: [C, n_bands, n_time] complex64 / complex128 (an STFT, CWT or Stockwell panel of C <= 64 records); weights:
    [n_bands, nbeam, C] of the same dtype -- beam_weights' or any others: the call is a general per-bin mixing of the records.
    -> beams [nbeam, n_bands, n_time].  NumPy panel in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    lib = _lib.require_gpu()
    z, was_numpy, rdtype = _matrix_stack(panel, "panel", "[C, bands, time]", square=False)
    n_ch, n_f, n_t = z.shape
    w, _, w_rdtype = _matrix_stack(weights, "weights", "[bands, beams, C]", square=False)
    if w_rdtype != rdtype or w.shape[0] != n_f or w.shape[2] != n_ch:
        raise ValueError(f"weights must be {z.dtype} [{n_f}, beams, {n_ch}] for this panel, got {w.dtype} {tuple(w.shape)}")
    dev, code = z.device, _lib.dtype_code(rdtype)
    w = w.to(dev)
    n_k = w.shape[1]
    out = torch.empty((n_k, n_f, n_t), dtype=z.dtype, device=dev)
    _lib.call(lib.qi_beam_steer, dev, code, dev.index, _lib.ptr(z), n_ch, n_f, n_t, _lib.ptr(w), n_k, _lib.ptr(out))
    return finish(out, was_numpy, False)


def _record_shape(a, what="signal", nonempty=True):
    """Shape (n,) or (C, n) of records, NumPy or tensor, checked before anything needs the device; n is its last entry."""
    shape = tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)
    if len(shape) not in (1, 2):
        raise ValueError(f"{what} must be 1-D [n] or 2-D [channels, n], got shape {shape}")
    if nonempty and shape[-1] < 1:
        raise ValueError("a record must hold at least one sample")
    return shape


def _records_and_timestamps(sig, timestamps, what="signal", shape=None):
    """Shape checks, the library and the uploads shared by interp_to_grid, cumulative_trapezoid and derivative -> (library,
    records [C, n] on the device, timestamps float64 on the device or None, its stride for the C call, was_numpy, was_1d)."""
    shape = shape or _record_shape(sig, what)  # (shape: of a caller that has checked the records already)
    n = shape[-1]
    if timestamps is not None and tuple(np.shape(timestamps)) not in ((n,), shape):
        raise ValueError(f"timestamps must be [n] or match the records' shape {shape}, got shape {tuple(np.shape(timestamps))}")
    lib = _lib.require_gpu()
    x, was_numpy, was_1d = as_signal(sig)
    t = None
    if timestamps is not None:
        if not isinstance(timestamps, torch.Tensor):
            timestamps = torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.float64))
        t = timestamps.to(device=x.device, dtype=torch.float64).contiguous()
    return lib, x, t, (n if t is not None and t.dim() == 2 else 0), was_numpy, was_1d


_IIR_FORMS = {"ba": _lib.QI_IIR_BA, "sos": _lib.QI_IIR_SOS, _lib.QI_IIR_BA: _lib.QI_IIR_BA, _lib.QI_IIR_SOS: _lib.QI_IIR_SOS}


def zero_phase_filter(sig, form, coef, zi, edge, taper=None):
    """Zero-phase IIR filter of records [n] or [C, n] (qi_filtfilt): scipy.signal.filtfilt's / sosfiltfilt's result for
    the same tables, float64 whatever the records' type.  form "ba": coef [2, order + 1] = (b, a) with a[0] = 1, zi [order]
    (iir_design.lfilter_zi), order <= 16; form "sos": coef [sections, 6], zi [sections, 2] (iir_design.sosfilt_zi), at most
    16 sections.  edge: samples of odd extension at each end (iir_design.filtfilt_edge / sosfiltfilt_edge); a record must
    be longer.  taper: [n] float64 multiplied into every record first (NumPy or a tensor), or None.  NumPy in -> NumPy
    out, CUDA tensor in -> CUDA tensor out on the current stream, nothing synchronised.  One lane per record: fewer than
    64 records take as long as 64."""
    if form not in _IIR_FORMS:
        raise ValueError(f'form must be "ba" or "sos", got {form!r}')
    code = _IIR_FORMS[form]
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    zi = np.ascontiguousarray(zi, dtype=np.float64)
    if code == _lib.QI_IIR_BA:
        if coef.ndim != 2 or coef.shape[0] != 2 or not 2 <= coef.shape[1] <= _lib.IIR_MAX + 1:
            raise ValueError(f"coef must be [2, order + 1] with order 1 .. {_lib.IIR_MAX}, got shape {coef.shape}")
        sections, order = 1, coef.shape[1] - 1
        if zi.shape != (order,):
            raise ValueError(f"zi must hold {order} values, got shape {zi.shape}")
        if coef[1, 0] != 1.0:
            raise ValueError("a[0] must be 1: normalise the coefficients")
    else:
        if coef.ndim != 2 or coef.shape[1] != 6 or not 1 <= coef.shape[0] <= _lib.IIR_MAX:
            raise ValueError(f"coef must be [sections, 6] with 1 .. {_lib.IIR_MAX} sections, got shape {coef.shape}")
        sections, order = coef.shape[0], 2
        if zi.shape != (sections, 2):
            raise ValueError(f"zi must be [{sections}, 2], got shape {zi.shape}")
        if not (coef[:, 3] == 1.0).all():
            raise ValueError("sos[:, 3] should be all ones")
    edge = int(edge)
    n = _record_shape(sig, nonempty=False)[-1]
    if edge < 0 or n <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    if taper is not None and tuple(taper.shape) != (n,):
        raise ValueError(f"taper must hold {n} values, got shape {tuple(taper.shape)}")
    lib = _lib.require_gpu()
    x, was_numpy, was_1d = as_signal(sig)
    dev = x.device
    n_ch = x.shape[0]
    out = torch.empty((n_ch, n), dtype=torch.float64, device=dev)
    if n_ch == 0:
        return finish(out, was_numpy, was_1d)
    if taper is not None:
        if not isinstance(taper, torch.Tensor):
            taper = torch.from_numpy(np.ascontiguousarray(taper, dtype=np.float64))
        taper = taper.to(device=dev, dtype=torch.float64).contiguous()
    scratch, nbytes = _lib.scratch(lib.qi_filtfilt_scratch_bytes, dev, n_ch, n, edge)
    _lib.call(lib.qi_filtfilt, dev, _lib.dtype_code(x.dtype), dev.index, _lib.ptr(x), n_ch, n, _lib.ptr(taper), code, sections, order,
              coef.ctypes.data_as(_lib._D), zi.ctypes.data_as(_lib._D), edge, _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, was_1d)


def zero_phase_decimate(sig, q, sos, zi, edge):
    """Zero-phase low-pass of records [n] or [C, n] and every q-th sample of the result, in one call (qi_decimate):
    scipy.signal.decimate(x, q, zero_phase=True)'s result for the same sections, ceil(n / q) samples per record.  The
    records' type is the type of all arithmetic and of the result: float32 stays float32 (SciPy's float32 bits), float64
    stays float64, anything else is filtered as float64.  sos [sections, 6] with sos[:, 3] = 1, at most 16 sections, and
    zi [sections, 2] (iir_design.decimator) are cast to that type.  edge: samples of odd extension at each end; a record
    must be longer.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out on the current stream, nothing
    synchronised.  One lane per record: a record is sequential in time, so one record takes 0.4 (float64) to 0.8 (float32)
    of the time of 64, and 64 take as long as 1024."""
    q = operator.index(q)
    if q < 1:
        raise ValueError(f"the decimation factor must be a positive integer, got {q}")
    edge = int(edge)
    n = _record_shape(sig, nonempty=False)[-1]
    if edge < 0 or n <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    sos = np.asarray(sos)
    zi = np.asarray(zi)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= _lib.IIR_MAX:
        raise ValueError(f"sos must be [sections, 6] with 1 .. {_lib.IIR_MAX} sections, got shape {sos.shape}")
    if zi.shape != (sos.shape[0], 2):
        raise ValueError(f"zi must be [{sos.shape[0]}, 2], got shape {zi.shape}")
    if not (sos[:, 3] == 1.0).all():
        raise ValueError("sos[:, 3] should be all ones")
    lib = _lib.require_gpu()
    x, was_numpy, was_1d = as_signal(sig)
    real = np.float64 if x.dtype == torch.float64 else np.float32
    sos = np.ascontiguousarray(sos, dtype=real)
    zi = np.ascontiguousarray(zi, dtype=real)
    dev = x.device
    n_ch = x.shape[0]
    out = torch.empty((n_ch, -(-n // q)), dtype=x.dtype, device=dev)
    if n_ch == 0:
        return finish(out, was_numpy, was_1d)
    code = _lib.dtype_code(x.dtype)
    scratch, nbytes = _lib.scratch(lib.qi_decimate_scratch_bytes, dev, code, n_ch, n, edge)
    _lib.call(lib.qi_decimate, dev, code, dev.index, _lib.ptr(x), n_ch, n, q, sos.shape[0], sos.ctypes.data, zi.ctypes.data, edge,
              _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, was_1d)


PEAK_SCALES = {"sigmax": _lib.QI_PEAK_SIGMAX, "sigmin": _lib.QI_PEAK_SIGMIN, "sigabs": _lib.QI_PEAK_SIGABS,
               "log2": _lib.QI_PEAK_LOG2, "log2max": _lib.QI_PEAK_LOG2MAX}
PEAK_HEIGHTS = {"none": _lib.QI_PEAK_HEIGHT_NONE, "abs": _lib.QI_PEAK_HEIGHT_ABS, "below_max": _lib.QI_PEAK_HEIGHT_BELOW_MAX,
                "below_raw_max": _lib.QI_PEAK_HEIGHT_BELOW_RAW_MAX}


def find_peaks(sig, scale, height_kind="none", height=0.0, want_scaled=False, capacity=None):
    """Scale records [n] or [C, n] and pick their peaks on the device (qi_find_peaks): scipy.signal.find_peaks(s,
    height=...)'s positions for s = the record scaled as utilities.picker.scale_signal_by_extraction_type scales it.
    scale: "sigmax", "sigmin", "sigabs" (s in the record's type), "log2", "log2max" (s in float64).  height_kind: "none";
    "abs" (s >= height); "below_max" (s >= max(s) - height); "below_raw_max" (s >= max(record) - height), the maxima taken
    per record on the device.  float32 records stay float32, anything but float32 and float64 is read as float64.
    -> (positions int64 [C, capacity], values float64 [C, capacity], counts int64 [C][, scaled [C, n]]), device tensors on
    the current stream, nothing synchronised; C = 1 for a record [n].  Row r holds its counts[r] peaks in ascending order in
    its first columns and leaves the others unwritten; counts[r] is the number found even when it exceeds `capacity`
    (default (n - 1) // 2, the most a record can hold; 0 picks nothing and only counts)."""
    if scale not in PEAK_SCALES:
        raise ValueError(f"scale must be one of {sorted(PEAK_SCALES)}, got {scale!r}")
    if height_kind not in PEAK_HEIGHTS:
        raise ValueError(f"height_kind must be one of {sorted(PEAK_HEIGHTS)}, got {height_kind!r}")
    height = float(height)
    n = _record_shape(sig)[-1]
    capacity = (n - 1) // 2 if capacity is None else operator.index(capacity)
    if capacity < 0:
        raise ValueError(f"capacity must not be negative, got {capacity}")
    lib = _lib.require_gpu()
    x, _, _ = as_signal(sig)
    dev = x.device
    n_ch = x.shape[0]
    log = scale in ("log2", "log2max")
    positions = torch.empty((n_ch, capacity), dtype=torch.int64, device=dev)
    values = torch.empty((n_ch, capacity), dtype=torch.float64, device=dev)
    counts = torch.zeros((n_ch,), dtype=torch.int64, device=dev)
    scaled = torch.empty((n_ch, n), dtype=torch.float64 if log else x.dtype, device=dev) if want_scaled else None
    if n_ch > 0:
        code = _lib.dtype_code(x.dtype)
        scratch, nbytes = _lib.scratch(lib.qi_peaks_scratch_bytes, dev, code, n_ch, n)
        _lib.call(lib.qi_find_peaks, dev, code, dev.index, _lib.ptr(x), n_ch, n, PEAK_SCALES[scale], float(scales.EPSILON64),
                  PEAK_HEIGHTS[height_kind], height, _lib.ptr(scaled), _lib.ptr(positions) if capacity else None,
                  _lib.ptr(values) if capacity else None, capacity, _lib.ptr(counts), _lib.ptr(scratch), nbytes)
    return (positions, values, counts, scaled) if want_scaled else (positions, values, counts)


def interp_to_grid(values, timestamps, start, delta, m):
    """Linear interpolation of records with uneven timestamps onto the even grid start + i * delta, i < m (qi_interp_grid):
    np.interp(start + np.arange(m) * delta, timestamps, values) bit for bit, per record.  values [n] or [C, n]; timestamps
    [n], shared by all records, or [C, n], a row per record -- records from sensors with different clocks come onto one
    grid in one call.  Timestamps are read as float64 and expected non-decreasing (not checked, as np.interp).  float32
    values are read as they are, anything but float32 and float64 as float64.  -> float64 [m] or [C, m]: NumPy in -> NumPy
    out, CUDA tensor in -> CUDA tensor out on the current stream, nothing synchronised."""
    start, delta = float(start), float(delta)
    m = operator.index(m)
    if m < 0:
        raise ValueError(f"m must not be negative, got {m}")
    if not np.isfinite(start):
        raise ValueError(f"start must be finite, got {start}")
    if not (np.isfinite(delta) and delta > 0.0):
        raise ValueError(f"delta must be finite and positive, got {delta}")
    if timestamps is None:
        raise ValueError("timestamps must be given: [n] or the records' shape")
    lib, x, t, stride, was_numpy, was_1d = _records_and_timestamps(values, timestamps, "values")
    dev = x.device
    n_ch, n = x.shape
    out = torch.empty((n_ch, m), dtype=torch.float64, device=dev)
    if n_ch > 0 and m > 0:
        _lib.call(lib.qi_interp_grid, dev, _lib.dtype_code(x.dtype), dev.index, _lib.ptr(x), _lib.ptr(t), stride, n_ch, n, start,
                  delta, m, _lib.ptr(out))
    return finish(out, was_numpy, was_1d)


def fft_resample(sig, m):
    """Fourier resampling of records [n] or [C, n] to m samples (qi_resample_fft): scipy.signal.resample(sig, m, axis=-1)
    for real records, no window.  float32 records stay float32, anything but float32 and float64 is read as float64.  The
    call owns its scratch (a copy of the records and the two spectra).  NumPy in -> NumPy out, CUDA tensor in -> CUDA
    tensor out on the current stream, nothing synchronised."""
    m = operator.index(m)
    if m < 1:
        raise ValueError(f"the new length must be at least 1, got {m}")
    n = _record_shape(sig)[-1]
    lib = _lib.require_gpu()
    x, was_numpy, was_1d = as_signal(sig)
    dev = x.device
    n_ch = x.shape[0]
    out = torch.empty((n_ch, m), dtype=x.dtype, device=dev)
    if n_ch > 0:
        code = _lib.dtype_code(x.dtype)
        scratch, nbytes = _lib.scratch(lib.qi_resample_fft_scratch_bytes, dev, code, n_ch, n, m)
        _lib.call(lib.qi_resample_fft, dev, code, dev.index, _lib.ptr(x), n_ch, n, m, _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, was_1d)


def cumulative_trapezoid(sig, timestamps=None, dx=1.0):
    """scipy.integrate.cumulative_trapezoid(sig, x=timestamps | dx=dx, initial=0) along the last axis of records [n] or
    [C, n] (qi_cumtrapz).  timestamps [n], shared by all records, or [C, n], a row per record, read as float64: the result
    is float64 whatever the records' type, as SciPy's.  Without them the spacing is the constant dx and float32 records
    give a float32 result (dx rounded to float32 once: SciPy's result for a Python float).  Anything but float32 and
    float64 is read as float64.  The terms are SciPy's bit for bit; they are added in the fixed tree of include/qi_tfr.h,
    which depends on the record length alone -- a record gives the same bits alone and in any batch -- not in NumPy's
    left-to-right order.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out on the current stream, nothing
    synchronised; the call owns its scratch (one value per 4096 samples and record)."""
    dx = float(dx)
    lib, x, t, stride, was_numpy, was_1d = _records_and_timestamps(sig, timestamps)
    dev = x.device
    n_ch, n = x.shape
    out = torch.empty((n_ch, n), dtype=torch.float64 if t is not None else x.dtype, device=dev)
    if n_ch > 0:
        code = _lib.dtype_code(x.dtype)
        scratch, nbytes = _lib.scratch(lib.qi_cumtrapz_scratch_bytes, dev, code, n_ch, n)
        _lib.call(lib.qi_cumtrapz, dev, code, dev.index, _lib.ptr(x), _lib.ptr(t), stride, dx, n_ch, n, _lib.ptr(out),
                  _lib.ptr(scratch), nbytes)
    return finish(out, was_numpy, was_1d)


DERIVATIVE_KINDS = {"gradient": _lib.QI_DERIV_GRADIENT, "difference": _lib.QI_DERIV_DIFFERENCE}


def derivative(sig, timestamps=None, h=1.0, kind="gradient", fill_at="end"):
    """Derivative of records [n] or [C, n] along the last axis (qi_derivative), NumPy's bits.  timestamps as in
    cumulative_trapezoid.
    kind "gradient": np.gradient(sig, h) or np.gradient(sig, timestamps) with edge_order 1, in the records' type (float32
    records over float64 timestamps are computed in float64 and stored as float32, as NumPy does).  The timestamps take
    NumPy's formula for uneven spacing; np.gradient itself switches to the even one when all their differences are equal
    (utilities.calculations.derivative_with_gradient_timestamps_s looks and passes h then).  At least two samples.
    kind "difference": np.diff(sig) * h -- h is the factor here, the sample rate, as the reference multiplies by it -- in the
    records' type, or np.diff(sig) / np.diff(timestamps) in float64: n - 1 values in a result of n columns, the first of
    them ("start") or the last ("end", fill_at) holding 0 for the caller's fill.
    Anything but float32 and float64 is read as float64.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out on the
    current stream, nothing synchronised."""
    if kind not in DERIVATIVE_KINDS:
        raise ValueError(f"kind must be one of {sorted(DERIVATIVE_KINDS)}, got {kind!r}")
    if fill_at not in ("start", "end"):
        raise ValueError(f"fill_at must be 'start' or 'end', got {fill_at!r}")
    h = float(h)
    difference = kind == "difference"
    shape = _record_shape(sig)
    if not difference and shape[-1] == 1:
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.")
    lib, x, t, stride, was_numpy, was_1d = _records_and_timestamps(sig, timestamps, shape=shape)
    dev = x.device
    n_ch, n = x.shape
    out = torch.empty((n_ch, n), dtype=torch.float64 if difference and t is not None else x.dtype, device=dev)
    offset = 1 if difference and fill_at == "start" else 0
    if n_ch > 0:
        _lib.call(lib.qi_derivative, dev, _lib.dtype_code(x.dtype), dev.index, DERIVATIVE_KINDS[kind], _lib.ptr(x), _lib.ptr(t),
                  stride, h, n_ch, n, _lib.ptr(out), offset)
        if difference:
            out[:, 0 if offset else n - 1] = 0
    return finish(out, was_numpy, was_1d)


SYNTH_KINDS = {name: code for code, name in enumerate(_lib.SYNTH_KINDS)}
SYNTH_AXES = {"rate": _lib.QI_AXIS_RATE, "step": _lib.QI_AXIS_STEP, "timestamps": _lib.QI_AXIS_TIMESTAMPS}
SYNTH_ENVELOPES = {"none": _lib.QI_ENVELOPE_NONE, "tukey": _lib.QI_ENVELOPE_TUKEY, "gate": _lib.QI_ENVELOPE_GATE}


def _synth_axis(axis, n):
    """("rate", rate[, s0[, s1]]), ("step", step[, s0[, s1]]) or ("timestamps", x[, s0[, s1]]) -> (code, value, x, s0, s1), host
    checks only: x stays what the caller gave ([n] or [C, n], NumPy or tensor)."""
    if not isinstance(axis, (tuple, list)) or not 2 <= len(axis) <= 4 or axis[0] not in SYNTH_AXES:
        raise ValueError(f"axis must be (form, value[, s0[, s1]]) with form one of {sorted(SYNTH_AXES)}, got {axis!r}")
    s0 = float(axis[2]) if len(axis) > 2 else 0.0
    s1 = float(axis[3]) if len(axis) > 3 else 0.0
    if axis[0] == "timestamps":
        shape = tuple(np.shape(axis[1]))
        if len(shape) not in (1, 2) or shape[-1] != n:
            raise ValueError(f"timestamps must be [n] or [records, n] with n = {n}, got shape {shape}")
        return SYNTH_AXES["timestamps"], 0.0, axis[1], s0, s1
    value = float(axis[1])
    if axis[0] == "rate" and value == 0.0:
        raise ValueError("the rate must not be 0")
    return SYNTH_AXES[axis[0]], value, None, s0, s1


def synth_time(k, axis):
    """The time of sample k as the kernels round it, in Python floats: t = (base(k) - s0) - s1 for an index form of `axis`."""
    form, value = axis[0], float(axis[1])
    s0 = float(axis[2]) if len(axis) > 2 else 0.0
    s1 = float(axis[3]) if len(axis) > 3 else 0.0
    return ((float(k) / value if form == "rate" else float(k) * value) - s0) - s1


def gate_span(n, axis, tmin, tmax):
    """(k0, m) of benchmark_signals.signal_gate on n samples of `axis`: the first sample with tmin <= t <= tmax and how many
    there are.  Index forms (non-decreasing in k for a positive rate or step): two bisections with the kernel's own t(k);
    shared timestamps [n]: counted."""
    if axis[0] == "timestamps":
        s0 = float(axis[2]) if len(axis) > 2 else 0.0
        s1 = float(axis[3]) if len(axis) > 3 else 0.0
        x = axis[1].detach().cpu().numpy() if isinstance(axis[1], torch.Tensor) else np.asarray(axis[1], dtype=np.float64)
        if x.ndim != 1:
            raise ValueError("a gate needs one time axis for all records: shared timestamps [n] or an index form")
        t = (x - s0) - s1
        include = np.logical_and(t >= tmin, t <= tmax)
        m = int(include.sum())
        k0 = int(np.argmax(include)) if m else 0
        if m and not include[k0:k0 + m].all():
            raise ValueError("the gate's samples must be consecutive: timestamps in ascending order")
        return k0, m
    if not float(axis[1]) > 0.0:
        raise ValueError("a gate needs a positive rate or step")

    def first(pred):  # the first k in [0, n] where pred(t(k)) holds; pred is monotone in k
        lo, hi = 0, n
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(synth_time(mid, axis)):
                hi = mid
            else:
                lo = mid + 1
        return lo

    k0 = first(lambda t: t >= tmin)
    k1 = first(lambda t: t > tmax)
    return (k0, k1 - k0) if k1 > k0 else (0, 0)


def _param_rows(params, width, what):
    rows = np.ascontiguousarray(params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else params, dtype=np.float64)
    if rows.ndim not in (1, 2) or rows.shape[-1] > width or rows.shape[-1] < 1:
        raise ValueError(f"{what} must be [p] or [records, p] with 1 <= p <= {width}, got shape {rows.shape}")
    padded = np.zeros(rows.shape[:-1] + (width,))
    padded[..., :rows.shape[-1]] = rows
    return padded


def _rows_and_axis(params, width, n, axis, records, device):
    """Host checks of synthesize and doppler, then the library and the uploads -> (lib, device, parameter rows on the
    device, their stride, C, 1-D result?, axis code, value, timestamps on the device or None, their stride, s0, s1)."""
    n = operator.index(n)
    if n < 1:
        raise ValueError("a record must hold at least one sample")
    rows = _param_rows(params, width, "params")
    code, value, x, s0, s1 = _synth_axis(axis, n)
    counts = {c for c in (rows.shape[0] if rows.ndim == 2 else None, np.shape(x)[0] if x is not None and np.ndim(x) == 2 else None,
                          None if records is None else operator.index(records)) if c is not None}
    if len(counts) > 1:
        raise ValueError(f"the parameter rows, the timestamp rows and `records` disagree on the record count: {sorted(counts)}")
    one = not counts
    n_ch = counts.pop() if counts else 1
    if n_ch < 0:
        raise ValueError(f"records must not be negative, got {n_ch}")
    lib = _lib.require_gpu()
    if device is None:
        device = x.device if isinstance(x, torch.Tensor) and x.is_cuda else default_device()
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    # through page-locked memory: a copy from pageable memory holds the host until the current stream has run it, and these
    # calls promise to synchronise nothing (the pinned block is PyTorch's to reuse once the copy has run)
    p = torch.from_numpy(rows).pin_memory().to(device, non_blocking=True)
    t = None
    if x is not None:
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        t = x.to(device=device, dtype=torch.float64).contiguous()
    return (lib, device, p, width if rows.ndim == 2 else 0, n_ch, one, code, value, t, n if t is not None and t.dim() == 2 else 0,
            s0, s1)


def synthesize(kind, params, n, axis=("step", 1.0), envelope=None, dtype=torch.float64, device=None, complex_out=False, records=None):
    """Records from a closed formula, made on the device (qi_synth; the formulas are spelled out in include/qi_tfr.h): the
    batch path of the synth package.  kind: one of SYNTH_KINDS.  params: the kind's float64 parameter row [p] -- one for
    all records -- or a row per record [C, p], p <= 12 (missing values are 0).  axis: ("rate", rate), ("step", step) or
    ("timestamps", x) with x [n] or [C, n], optionally followed by s0 and s1: t = (base(k) - s0) - s1.  envelope: None,
    ("tukey", alpha) -- a Tukey window over the whole record -- or ("gate", tmin, tmax, alpha) -- benchmark_signals.signal_gate,
    which needs one time axis for all records.  dtype: the stored type, float32 or float64; every sample is evaluated in
    float64 and rounded once.  complex_out: a complex tensor ("quantum_chirp"; the other kinds have no imaginary part).
    records: the record count when neither params nor timestamps have rows (every record the same).
    -> a tensor [C, n] on `device` ([n] when nothing gave a record count), on the current stream, nothing synchronised."""
    if kind not in SYNTH_KINDS:
        raise ValueError(f"kind must be one of {sorted(SYNTH_KINDS)}, got {kind!r}")
    rdtype = _real_dtype(dtype)
    n = operator.index(n)
    env, alpha, tmin, tmax, k0, m = SYNTH_ENVELOPES["none"], 0.0, 0.0, 0.0, 0, 0
    if envelope is not None:
        if not isinstance(envelope, (tuple, list)) or not envelope or envelope[0] not in ("tukey", "gate") or \
                len(envelope) != (2 if envelope[0] == "tukey" else 4):
            raise ValueError(f'envelope must be None, ("tukey", alpha) or ("gate", tmin, tmax, alpha), got {envelope!r}')
        env = SYNTH_ENVELOPES[envelope[0]]
        alpha = float(envelope[-1])
        if envelope[0] == "gate":
            tmin, tmax = float(envelope[1]), float(envelope[2])
            if n >= 1:
                _synth_axis(axis, n)
                k0, m = gate_span(n, axis, tmin, tmax)
    lib, dev, p, p_stride, n_ch, one, code, value, t, t_stride, s0, s1 = _rows_and_axis(params, _lib.SYNTH_PARAMS, n, axis, records, device)
    out = torch.empty((n_ch, n), dtype=_complex_of(rdtype) if complex_out else rdtype, device=dev)
    if n_ch > 0:
        _lib.call(lib.qi_synth, dev, _lib.dtype_code(rdtype), dev.index, SYNTH_KINDS[kind], int(bool(complex_out)), _lib.ptr(p), p_stride,
                  code, value, _lib.ptr(t), t_stride, s0, s1, env, alpha, tmin, tmax, k0, m, n_ch, n, _lib.ptr(out))
    return out[0] if one else out


def doppler(params, n, axis, inverse=False, device=None, records=None):
    """Source / receiver geometry of synth.doppler on the device (qi_doppler): doppler._get_final_vals for a row of times per
    record.  params: [12] or [C, 12] float64 -- c, c**2, 1. / (c**2 - speed**2), the source velocity, the receiver velocity,
    the initial range receiver - source (synth.doppler.geometry_row builds one) -- a row per receiver computes an array of
    receivers in one call.  axis, records: as for synthesize.  -> (time, range, omega over omega_c), float64 tensors [C, n]
    ([n] when nothing gave a record count) on the current stream, nothing synchronised."""
    if np.shape(params)[-1:] != (_lib.DOPPLER_PARAMS,):
        raise ValueError(f"params must be [{_lib.DOPPLER_PARAMS}] or [records, {_lib.DOPPLER_PARAMS}], got shape {tuple(np.shape(params))}")
    lib, dev, p, p_stride, n_ch, one, code, value, t, t_stride, s0, s1 = _rows_and_axis(params, _lib.DOPPLER_PARAMS, n, axis, records, device)
    n = operator.index(n)
    outs = [torch.empty((n_ch, n), dtype=torch.float64, device=dev) for _ in range(3)]
    if n_ch > 0:
        _lib.call(lib.qi_doppler, dev, dev.index, int(bool(inverse)), _lib.ptr(p), p_stride, code, value, _lib.ptr(t), t_stride, s0, s1,
                  n_ch, n, *(_lib.ptr(o) for o in outs))
    return tuple(o[0] for o in outs) if one else tuple(outs)


# What the reference-signature wrappers hand back to NumPy callers for float32 records.  The reference returns
# complex128 panels (float64 bits) whatever the record's dtype (styx_cwt.py:195-198, styx_stx.py:228,
# cwt_atoms.py:408): "reference" computes in float32 and widens on the way out, so a drop-in caller sees the
# reference's dtypes; "native" keeps complex64 / float32 (half the host memory and copy time).  CUDA tensors in ->
# tensors out are never widened.
NUMPY_RESULT_DTYPE = "reference"


def finish(result_tensor, was_numpy, was_1d, widen=False):
    """Undo as_signal's batching / device move on an output.  widen: a panel the reference would return in double
    precision (see NUMPY_RESULT_DTYPE).  NumPy callers get an array backed by page-locked memory (the copy from the
    device then runs at PCIe speed instead of through a pageable staging buffer); the widening runs on the device."""
    if result_tensor is None:
        return None
    t = result_tensor[0] if was_1d else result_tensor
    if not was_numpy:
        return t
    t = t.contiguous()
    if widen and NUMPY_RESULT_DTYPE == "reference" and t.dtype in (torch.complex64, torch.float32) and t.numel() > 0:
        wide = torch.empty(t.shape, dtype=torch.complex128 if t.dtype == torch.complex64 else torch.float64, device=t.device)
        src = torch.view_as_real(t) if t.is_complex() else t
        _lib.call(_lib.load().qi_widen, t.device, t.device.index, _lib.ptr(src), _lib.ptr(wide), src.numel())
        t = wide
    nbytes = t.numel() * t.element_size()
    if nbytes >= PINNED_RESULT_MAX_BYTES:
        return _staged_copy(t)  # bounded page-locked memory: two 64 MiB staging buffers, pageable result
    if nbytes >= (1 << 20):
        # the result itself in page-locked memory: one copy at PCIe speed.  PyTorch's pinned allocator keeps freed blocks
        # page-locked, so what it has cached is handed back to the system once it exceeds the cap.
        _trim_pinned_cache()
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        host.copy_(t)
        return host.numpy()
    return t.cpu().numpy()


PINNED_RESULT_MAX_BYTES = 4 << 30  # larger results are staged through two fixed buffers into pageable memory
STAGE_PIECE_BYTES = 64 << 20  # bytes per staged piece (<= the 64 MiB staging buffers; tests lower it to exercise many pieces)


def _trim_pinned_cache():
    """Return cached (freed, still page-locked) host blocks to the system when they exceed PINNED_RESULT_MAX_BYTES."""
    try:
        stats = torch.cuda.memory.host_memory_stats()
        cached = int(stats.get("allocated_bytes.current", 0)) - int(stats.get("active_bytes.current", 0))
        if cached > PINNED_RESULT_MAX_BYTES:
            torch._C._host_emptyCache()
    except Exception:  # (older PyTorch: no host allocator statistics -- nothing to trim with)
        pass


_STAGE_BYTES = 64 << 20
_STAGE = []  # two page-locked staging buffers, made once (PyTorch's pinned allocator never unpins what it freed)
_STAGE_LOCK = threading.Lock()  # the two buffers are shared by every caller of finish(): one staged copy at a time
_NUMPY_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128,
             torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}


def _staged_copy(t):
    """Device tensor -> pageable NumPy array through two fixed page-locked buffers: the device-to-host copy of piece k + 1
    runs while piece k is copied out of its staging buffer, and no page-locked memory grows with the result (an order-12
    panel is 1.6 GB and more once widened)."""
    if t.dtype not in _NUMPY_OF:
        raise TypeError(f"no NumPy dtype for a {t.dtype} result")
    flat = t.reshape(-1).view(torch.uint8) if not t.is_complex() else torch.view_as_real(t).reshape(-1).view(torch.uint8)
    out = np.empty(t.shape, dtype=_NUMPY_OF[t.dtype])
    dst = torch.from_numpy(out.reshape(-1).view(np.uint8))
    total = flat.numel()
    stream = torch.cuda.current_stream(t.device)
    events = [torch.cuda.Event(), torch.cuda.Event()]
    piece = min(_STAGE_BYTES, max(int(STAGE_PIECE_BYTES), 4096))
    pieces = [(o, min(piece, total - o)) for o in range(0, total, piece)]
    with _STAGE_LOCK:
        if not _STAGE:
            _STAGE.extend(torch.empty(_STAGE_BYTES, dtype=torch.uint8, pin_memory=True) for _ in range(2))
        for k, (o, m) in enumerate(pieces):
            _STAGE[k & 1][:m].copy_(flat[o : o + m], non_blocking=True)
            events[k & 1].record(stream)
            if k:
                po, pm = pieces[k - 1]
                events[(k - 1) & 1].synchronize()
                dst[po : po + pm].copy_(_STAGE[(k - 1) & 1][:pm])
        po, pm = pieces[-1]
        events[(len(pieces) - 1) & 1].synchronize()
        dst[po : po + pm].copy_(_STAGE[(len(pieces) - 1) & 1][:pm])
    return out
