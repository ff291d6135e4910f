"""`mixdq_extension._C` for MI355X: the five operator entry points of the reference's pybind
module (csrc/main.cpp:9-13), same names, argument order, kwarg names and error behaviour, backed
by libmixdq_hip.so (include/mixdq_hip.h) through ctypes.

    quantize_per_tensor_to_int8(input, scale_inv, zero_point)              quantize.cc:9-30
    quantize_per_tensor_to_int8_vectorized(input, scale_inv, zero_point)   quantize.cc:32-53
    qlinear_w8_a8_ohalf(input_int8, weight_int8, weight_scale, input_scale, input_zero_point,
                        weight_sum_by_input_channels, scale, bias0, bias=None)   qlinear.cc:13-137
    qconv2d_w8_a8_ohalf(input_int8, weight_int8, weight_scale, input_scale, input_zero_point,
                        scale, weight_sum_by_input_channels, bias0, bias=None, stride=1,
                        padding=0, dilation=1)                               qconv2d.cc:27-206
    qlinear_fp_reference(input, weight, bias=None)                           qlinear.cc:140-204

PyTorch is plumbing here: device memory (torch.empty -> caching allocator, so hipGraph capture
works), the current stream and error propagation.  There is NO CPU or eager fallback: if the HIP
library is missing the import fails, and non-GPU tensors raise like the reference's TORCH_CHECKs.
"""
from __future__ import annotations

import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIXDQ_HIP_LIB") or os.path.join(_PKG, "libmixdq_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the HIP extension has not been built. Run "
        "`python -m mixdq_amd.build` (needs hipcc). There is no CPU fallback.")

_lib = ctypes.CDLL(LIB_PATH)

_vp, _i64, _i32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_lib.mixdq_status_string.restype = ctypes.c_char_p
_lib.mixdq_status_string.argtypes = [_i32]
_lib.mixdq_abi_version.restype = _i32
_lib.mixdq_quantize_f16_i8.argtypes = [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]
_lib.mixdq_qlinear_w8a8.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]
_lib.mixdq_qlinear_w8a8_rows.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32,
                                         _i32, _i32, _i32, _vp, _i64, _i32, _vp]
_lib.mixdq_qconv2d_workspace_bytes.restype = _sz
_lib.mixdq_qconv2d_workspace_bytes.argtypes = [_i32] * 4
_lib.mixdq_qconv2d_w8a8.argtypes = [_vp] * 9 + [_i32] * 11 + [_vp]
_lib.mixdq_conv_border_table.argtypes = [_vp, _vp, _i32, _i32, _i32, _vp]
_lib.mixdq_qconv2d_w8a8_table.argtypes = [_vp] * 8 + [_i32] * 9 + [_vp, _i64, _i32, _vp]
_lib.mixdq_conv_zero_point_propagate.argtypes = [_vp, _vp, _vp] + [_i32] * 8 + [_vp]
_lib.mixdq_gemm_f16.argtypes = [_vp, _vp, _vp, _i64, _i32, _i32, _vp]
for _n in ("mixdq_quantize_f16_i8", "mixdq_qlinear_w8a8", "mixdq_qlinear_w8a8_rows",
           "mixdq_qconv2d_w8a8", "mixdq_conv_border_table", "mixdq_qconv2d_w8a8_table",
           "mixdq_conv_zero_point_propagate", "mixdq_gemm_f16"):
    getattr(_lib, _n).restype = _i32

_lib.mixdq_igemm_select.argtypes = [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]
_lib.mixdq_igemm_select.restype = _i32

ABI_VERSION = _lib.mixdq_abi_version()
# This binding is written against ONE data-layout contract (include/mixdq_hip.h MIXDQ_ABI_VERSION: e.g. ABI 3
# stores GEMM+GEGLU weight rows as value|gate groups of 16 where ABI 2 had 32): a library of another
# version (MIXDQ_HIP_LIB A/B runs) would compute silently different tensors -- refuse it here.
EXPECTED_ABI = 3
if ABI_VERSION != EXPECTED_ABI:
    raise ImportError(f"{LIB_PATH} reports ABI version {ABI_VERSION}; mixdq_amd._C is written for "
                      f"ABI {EXPECTED_ABI} (rebuild with `python -m mixdq_amd.build --force`)")


_lib.mixdq_igemm_select_id.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_igemm_select_id.restype = _i32
_lib.mixdq_igemm_select_id_w4.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_igemm_select_id_w4.restype = _i32


_lib.mixdq_igemm_select_id_geglu.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_igemm_select_id_geglu.restype = _i32
_lib.mixdq_igemm_select_id_w2.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_igemm_select_id_w2.restype = _i32
_lib.mixdq_igemm_select_id_geglu_w2.argtypes = [_i64, _i32, _i32]
_lib.mixdq_igemm_select_id_geglu_w2.restype = _i32


def igemm_select_id(M: int, N: int, k_align: int, k_total: int = 0, w4: bool = False,
                    geglu: bool = False, w2: bool = False) -> int:
    """Configuration id (IGEMM_CONFIGS key) the automatic choice makes for this problem
    (`w4` / `w2`: for packed 4- / 2-bit weights, MIXDQ_FLAG_W4 / _W2; `geglu`: for the GEMM + GEGLU
    launch)."""
    _check(not (w4 and w2), "w4 and w2 are exclusive")
    if w2:
        if geglu:
            return int(_lib.mixdq_igemm_select_id_geglu_w2(M, N, k_total or k_align))
        return int(_lib.mixdq_igemm_select_id_w2(M, N, k_align, k_total or k_align))
    if geglu:
        return int(_lib.mixdq_igemm_select_id_geglu(M, N, k_total or k_align, int(w4)))
    if w4:
        return int(_lib.mixdq_igemm_select_id_w4(M, N, k_align, k_total or k_align))
    return int(_lib.mixdq_igemm_select_id(M, N, k_align, k_total or k_align))


def igemm_select(M: int, N: int, k_align: int, k_total: int = 0):
    """(BM, BN, BK, STAGES) of the igemm_kernel instantiation used for this problem; zeros =
    the generic small-alignment kernel."""
    bm, bn, bk, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _status(_lib.mixdq_igemm_select(M, N, k_align, k_total or k_align, ctypes.byref(bm),
                                    ctypes.byref(bn),
                                    ctypes.byref(bk), ctypes.byref(st)), "igemm_select")
    return bm.value, bn.value, bk.value, st.value

# The tile tables, as the LOADED library reports them (mixdq_tile_config), not a copy of the tables in csrc/.
if not hasattr(_lib, "mixdq_tile_config"):
    raise ImportError(f"{LIB_PATH} does not export mixdq_tile_config; mixdq_amd._C reads its tile tables from the "
                      "library (rebuild with `python -m mixdq_amd.build --force`)")
_lib.mixdq_tile_config.argtypes = [_i32, _i32, _vp]
_lib.mixdq_tile_config.restype = _i32


def tile_family(family):
    """The rows (10 ints each) of one family of mixdq_tile_config."""
    row = (ctypes.c_int * 10)()
    rows = []
    for i in range(_lib.mixdq_tile_config(family, 0, None)):
        _lib.mixdq_tile_config(family, i, row)
        rows.append(tuple(row))
    return rows


_TILES = tile_family(0)
# Kernel configurations of the INT8 GEMM / conv family: id -> (BM, BN, BK, STAGES).  `_cfg=id` forces one (tuning
# and tests); 0 = automatic.
IGEMM_CONFIGS = {r[0]: r[1:5] for r in _TILES}
# id -> (WM, WN, KSPLIT, MT): wave grid, k-split groups and MFMA shape of each configuration (the template
# arguments that tell two configurations of one tile shape apart in a kernel trace)
IGEMM_WAVES = {r[0]: r[5:9] for r in _TILES}
# configuration ids a packed-W2 launch cannot take (csrc/igemm.hip w2_tile_ok)
W2_INADMISSIBLE = tuple(sorted(r[0] for r in _TILES if not r[9] & 2))
F16_CONFIGS = tuple(sorted(r[0] for r in tile_family(1)))       # the FP16 layers' tiles (one accumulation order)
GROUPED_CONFIGS = tuple(sorted(r[0] for r in tile_family(2)))   # the ids qlinear_grouped's _cfg takes
F16IN_CONFIGS = tuple(sorted(r[0] for r in tile_family(3)))     # the quantize-in-prologue family's tiles
# the LDS-halo conv's tiles: id -> output pixels (rows, columns), channels
HALO_TILES = {r[0]: r[1:4] for r in tile_family(5)}

FLAG_W4 = 2   # MIXDQ_FLAG_W4: the weight tensor holds packed signed 4-bit values
FLAG_W2 = 16  # MIXDQ_FLAG_W2: the weight tensor holds packed signed 2-bit values ([N, K/4])
FLAG_UPSAMPLE2X = 4   # MIXDQ_FLAG_UPSAMPLE2X: the conv input is read through a nearest 2x upsampling
FLAG_PAD_AFTER = 1 << 19   # MIXDQ_FLAG_PAD_AFTER: conv2d_f16's padding lies below and right of the image only
FLAG_CAUSAL = 32      # MIXDQ_FLAG_CAUSAL: attention_f16's causal mask (query row i attends to keys 0 .. i)
FLAG_ACT = {None: 0, "gelu": 64, "quick_gelu": 128}   # MIXDQ_FLAG_ACT_GELU / _QUICK_GELU: linear_f16's epilogue activation
# MIXDQ_FLAG_A4_<i>: quantizer slot i of a launch is a 4-bit one -- q clamped to [-128, -113] (Path A's [0, 15]
# shifted by -128); the GEMMs read the operand unchanged
FLAG_A4_0, FLAG_A4_1, FLAG_A4_2 = 1 << 16, 1 << 17, 1 << 18
FLAG_A4 = (FLAG_A4_0, FLAG_A4_1, FLAG_A4_2)
ACT_BITS = (8, 4)          # the activation widths the producers take


def _wflag(w4, w2):
    """MIXDQ_FLAG_W4 / _W2 for a launch on packed weights (never both)."""
    _check(not (w4 and w2), "_w4 and _w2 are exclusive")
    return FLAG_W2 if w2 else FLAG_W4 if w4 else 0


def _aflag(abits, slot=0):
    """MIXDQ_FLAG_A4_<slot> for a 4-bit quantizer, 0 for an 8-bit one."""
    _check(abits in ACT_BITS, f"activation bits must be 8 or 4, got {abits!r}")
    return FLAG_A4[slot] if abits == 4 else 0


def _kmul(w4, w2):
    """Weights per stored byte: K = weight.size(1) * _kmul(...)."""
    return 4 if w2 else 2 if w4 else 1


# Rounding variant of the fused multiply-adds: "A" (default) = FMA,
# "B" = separate multiply and add.  Read once at import; no other global state.
FLAGS = 1 if os.environ.get("MIXDQ_EPILOGUE_VARIANT", "A").upper() == "B" else 0


# Launch recorder (measurement only: bench.py's roofline leg, tools/).  While `RECORD` is a list,
# every INT8 GEMM / conv entry point appends (name, (M, N, K, k_align), w4, replay) to it, where
# replay() re-issues the very same launch on the same device tensors.  None = off (the default).
# Each entry is a Launch: that 4-tuple, plus `.wbits` -- 8, 4 or 2, the stored weight width (a W2 launch
# records w4 = False; its `.wbits` tells it apart).
RECORD = None


class Launch(tuple):
    """(name, (M, N, K, k_align), w4, replay) with the stored weight width as `.wbits`."""
    wbits = 8


def _record(name, M, N, K, k_align, w4, fn, args, kwargs, w2=False):
    if RECORD is None:
        return
    def replay():
        global RECORD
        saved, RECORD = RECORD, None
        try:
            return fn(*args, **kwargs)
        finally:
            RECORD = saved
    entry = Launch((name, (int(M), int(N), int(K), int(k_align)), bool(w4), replay))
    entry.wbits = 2 if w2 else 4 if w4 else 8
    RECORD.append(entry)


class PrefetchContext:
    """One forward's weight trace and prefetch plan (mixdq_amd/unet.py's planner).

    While a context is active on the calling THREAD (`with ctx:`), every GEMM / conv entry point appends the
    weight operand it was called with to `trace` and every long-key attention launch a marker -- the
    execution order of the network's weights relative to its self-attention launches -- and the i-th such
    attention launch carries `plan[i]` (weak references to weight tensors) as its payload.  The state lives
    in the object, never in the module: two UNets, or two threads each driving a device, keep their own.
    Only tensors on `device` are traced or handed to a launch (a payload address of another device would be
    dereferenced by the kernel).  A context does not nest: entering one while another is active on the
    thread leaves the outer one in charge and makes the inner one a no-op."""
    __slots__ = ("device", "trace", "plan", "att_index", "_outer", "_live")

    def __init__(self, device, plan=None):
        self.device = torch.device(device)
        self.trace = []
        self.plan = plan
        self.att_index = 0
        self._outer = None
        self._live = False

    def __enter__(self):
        self._outer = getattr(_TLS, "ctx", None)
        if self._outer is None:
            _TLS.ctx = self
            self._live = True
        return self

    def __exit__(self, *exc):
        if self._live:
            _TLS.ctx = None
            self._live = False
        return False

    def payload(self):
        """The tensors of the next long-key attention launch (dead references and other devices dropped)."""
        i, self.att_index = self.att_index, self.att_index + 1
        if self.plan is None or i >= len(self.plan):
            return None
        out = []
        for ref in self.plan[i]:
            t = ref()
            if t is not None and t.device == self.device:
                out.append(t)
        return out


import threading as _threading   # noqa: E402
import weakref as _weakref       # noqa: E402, F401  (plans hold weakref.ref(tensor))
_TLS = _threading.local()


def prefetch_context():
    """The PrefetchContext active on this thread, or None."""
    return getattr(_TLS, "ctx", None)


def _trace_w(t):
    ctx = getattr(_TLS, "ctx", None)
    if ctx is not None and t is not None and t.device == ctx.device:
        ctx.trace.append(t)


def _check(cond: bool, msg: str):
    if not cond:
        raise RuntimeError(msg)


def _status(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what}: {_lib.mixdq_status_string(code).decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i64arr(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _f32vec(t: torch.Tensor) -> torch.Tensor:
    """Per-channel epilogue vectors are read with 16-byte loads: contiguous and aligned."""
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _quantize(input, scale_inv, zero_point, abits=8):
    _check(input.is_cuda, "input should be on CUDA")
    _check(input.device == scale_inv.device, "input and scale should be on the same device")
    _check(input.device == zero_point.device,
           "input and zero_point should be on the same device")
    _check(input.dtype == torch.float16, "input should be fp16")
    _check(scale_inv.dtype == torch.float32, "scale_inv should be fp32")
    _check(zero_point.dtype == torch.float32, "zero_point should be fp32")
    out = torch.empty_like(input, dtype=torch.int8)
    if input.numel() == 0:
        return out
    nd = input.dim()
    sizes = list(input.shape) if nd else [1]
    xs = list(input.stride()) if nd else [1]
    os_ = list(out.stride()) if nd else [1]
    with torch.cuda.device(input.device):
        code = _lib.mixdq_quantize_f16_i8(input.data_ptr(), out.data_ptr(), _i64arr(sizes),
                                          _i64arr(xs), _i64arr(os_), len(sizes),
                                          scale_inv.data_ptr(), zero_point.data_ptr(),
                                          FLAGS | _aflag(abits), _stream())
    _status(code, "quantize_per_tensor_to_int8")
    return out


if not hasattr(_lib, "mixdq_quantize_f16_i8_route"):
    raise ImportError(f"{LIB_PATH} does not export mixdq_quantize_f16_i8_route (rebuild with "
                      "`python -m mixdq_amd.build --force`)")
_lib.mixdq_quantize_f16_i8_route.argtypes = [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.mixdq_quantize_f16_i8_route.restype = _i32
QUANTIZE_ROUTES = {-1: "none", 0: "dense", 1: "rows", 2: "scalar"}


def quantize_route(sizes, x_strides, out_strides, x_ptr: int, out_ptr: int):
    """What mixdq_quantize_f16_i8 launches for this call, asked of the library (no GPU needed; the pointers are
    looked at for alignment only): (status, route name, collapsed rank, the four collapsed sizes, blocks)."""
    nd = len(sizes)
    route, rank, blocks = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(0)
    sz4 = (ctypes.c_int64 * 4)()
    code = _lib.mixdq_quantize_f16_i8_route(_i64arr(list(sizes) or [1]), _i64arr(list(x_strides) or [1]),
                                            _i64arr(list(out_strides) or [1]), nd or 1, x_ptr, out_ptr,
                                            ctypes.byref(route), ctypes.byref(rank), sz4, ctypes.byref(blocks))
    return int(code), QUANTIZE_ROUTES[route.value], rank.value, tuple(sz4), blocks.value


def quantize_per_tensor_to_int8(input, scale_inv, zero_point, *, _abits=8):
    """Quantize to int 8 per tensor with scale and zero point.  `_abits=4`: a 4-bit activation quantizer
    (MIXDQ_FLAG_A4_0): the same INT8 operand clamped to [-128, -113]."""
    return _quantize(input, scale_inv, zero_point, _abits)


def quantize_per_tensor_to_int8_vectorized(input, scale_inv, zero_point, *, _abits=8):
    """Same kernel family as quantize_per_tensor_to_int8 (every path here is vectorised)."""
    return _quantize(input, scale_inv, zero_point, _abits)


def qlinear_w8_a8_ohalf(input_int8, weight_int8, weight_scale, input_scale, input_zero_point,
                        weight_sum_by_input_channels, scale, bias0, bias=None, *,
                        _out=None, _row_map=None, _cfg=0, _residual=None, _residual_div=1,
                        _w4=False, _w2=False):
    _trace_w(weight_int8)
    _check(input_int8.is_cuda, "Input should be on GPU.")
    dev = input_int8.device
    _check(dev == weight_int8.device, "input and weight_int8 should be on the same device.")
    _check(dev == weight_scale.device, "input and weight_scale should be on the same device.")
    _check(dev == input_scale.device, "input and input_scale should be on the same device.")
    _check(dev == input_zero_point.device,
           "input and input_zero_point should be on the same device.")
    _check(dev == weight_sum_by_input_channels.device,
           "input and input_zero_point should be on the same device.")
    if bias is not None:
        _check(dev == bias.device, "input and bias should be on the same device.")
    _check(input_int8.dtype == torch.int8, "input_int8 should be int8 type")
    _check(weight_int8.dtype == torch.int8, "weight_int8 should be int8 type")
    _check(weight_scale.dtype == torch.float32,
           "Currently only support weight_scale with float32 type")
    _check(input_scale.dtype == torch.float32,
           "Currently only support input_scale with float32 type")
    _check(input_zero_point.dtype == torch.float32,
           "Currently only support input_zero_point with float32 type")
    _check(weight_sum_by_input_channels.dtype == torch.float32,
           "Currently only support weight_sum_by_input_channels with float32 type")
    if bias is not None:
        _check(bias.dtype == torch.float16, "Currently only support bias with float16 type")
    _check(scale.dtype == torch.float32 and bias0.dtype == torch.float32,
           "scale and bias0 should be float32")
    wflag = _wflag(_w4, _w2)
    N, K = weight_int8.size(0), weight_int8.size(1) * _kmul(_w4, _w2)   # _w4 / _w2: packed
    _check(weight_scale.numel() == N,
           "The size of the weight_scale vector should be equal to output_channels.")
    _check(weight_sum_by_input_channels.numel() == N,
           "The size of weight_sum_by_input_channels should equal output_channels.")
    _check(scale.numel() == N and bias0.numel() == N,
           "The size of scale and bias0 should be equal to output_channels.")
    if bias is not None:
        _check(bias.numel() == N,
               "The size of the bias vector should be equal to output_channels.")
    _check(input_int8.size(-1) == K,
           f"The last dimension of input and weight should match, got {input_int8.size(-1)} "
           f"and {K}.")
    a = input_int8.contiguous()
    w = weight_int8.contiguous()
    M = a.numel() // K if K else 0
    D = _out if _out is not None else torch.empty(
        list(input_int8.shape[:-1]) + [N], dtype=torch.float16, device=dev)
    rm = _row_map or (0, 0, 0)
    sc, b0 = _f32vec(scale), _f32vec(bias0)
    bs = None if bias is None else bias.contiguous()
    if _residual is not None:
        _check(_residual.dtype == torch.float16 and _residual.is_contiguous()
               and _residual.numel() == (M // _residual_div) * N,
               "residual should be contiguous fp16 of M / residual_div rows")
    _record("linear", M, N, K, K, _w4, qlinear_w8_a8_ohalf,
            (input_int8, weight_int8, weight_scale, input_scale, input_zero_point,
             weight_sum_by_input_channels, scale, bias0, bias),
            dict(_out=_out, _row_map=_row_map, _cfg=_cfg, _residual=_residual,
                 _residual_div=_residual_div, _w4=_w4, _w2=_w2), w2=_w2)
    with torch.cuda.device(dev):
        code = _lib.mixdq_qlinear_w8a8_rows(a.data_ptr(), w.data_ptr(), b0.data_ptr(),
                                            sc.data_ptr(), _ptr(bs), D.data_ptr(), M, N, K,
                                            rm[0], rm[1], rm[2], _ptr(_residual), _residual_div,
                                            FLAGS | (_cfg << 8) | wflag,
                                            _stream())
    _status(code, "qlinear_w8_a8_ohalf")
    return D


_lib.mixdq_qlinear_f16in_w8a8.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32,
                                         _i32, _i32, _i32, _vp, _i64, _i32, _vp]
_lib.mixdq_qlinear_f16in_w8a8.restype = _i32
_lib.mixdq_qlinear_f16in_supported.argtypes = [_i64, _i32, _i32, _i64, _i64, _i32]
_lib.mixdq_qlinear_f16in_supported.restype = _i32
_lib.mixdq_qlinear_f16in_select_id.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_qlinear_f16in_select_id.restype = _i32
_lib.mixdq_qlinear_f16in_preferred.argtypes = [_i64, _i32, _i32, _i32]
_lib.mixdq_qlinear_f16in_preferred.restype = _i32

FLAG_A_ROWMAP = 8   # MIXDQ_FLAG_A_ROWMAP: the FP16 operand's rows follow the output row map

# Quantize-in-prologue (csrc/igemm_aq.hip): QuantizedLinear / 1x1 QuantizedConv2d hand their FP16 input
# straight to a GEMM that quantizes it in its staging path -- one launch where the reference has two
# (nn/Linear.py:162-176).  MIXDQ_F16IN=0 restores the reference's quantize launch (A/B runs, tests).
# "auto" (default): where the library's cost model expects the one launch to be cheaper
# (mixdq_qlinear_f16in_preferred: narrow layers -- the 1x1 shortcuts, K <= 640); "1": wherever supported.
F16IN = os.environ.get("MIXDQ_F16IN", "auto").lower()
F16IN = {"0": "0", "off": "0", "1": "1", "on": "1"}.get(F16IN, "auto")


def _rows_view(x: torch.Tensor, K: int):
    """(M, lda, leading shape) if `x` [..., K] can be read in place as M rows of K contiguous FP16 values
    a constant `lda` elements apart (a dense tensor, or a last-dimension slice of one), else None."""
    if x.dim() == 0 or x.size(-1) != K or (K > 1 and x.stride(-1) != 1):
        return None
    lead = list(x.shape[:-1])
    M = 1
    for d in lead:
        M *= d
    if M == 0:
        return None
    lda = None
    expect = None                      # stride the next-outer dimension must have
    for size, stride in zip(reversed(lead), reversed(x.stride()[:-1])):
        if size == 1:
            continue
        if lda is None:
            lda, expect = stride, stride * size
        elif stride != expect:
            return None
        else:
            expect = stride * size
    if lda is None:
        lda = K
    return M, lda, lead


def qlinear_f16in_supported(x: torch.Tensor, N: int, K: int, *, w4: bool = False, bos: bool = False,
                            w2: bool = False, abits: int = 8) -> bool:
    """True if qlinear_f16in takes `x` (fp16 [..., K]; bos: [B, T, K] whose tokens 1.. are the operand).
    Packed-W2 weights (`w2`) or a 4-bit activation quantizer (`abits=4`): never -- the quantizing family is
    not built for them; the caller quantizes and runs the GEMM."""
    if w2 or abits != 8:
        return False
    if not (x.is_cuda and x.dtype == torch.float16 and x.data_ptr() % 16 == 0):
        return False
    if bos:
        if x.dim() != 3 or not x.is_contiguous() or x.size(1) < 2:
            return False
        B, T = x.size(0), x.size(1)
        return bool(_lib.mixdq_qlinear_f16in_supported(B * (T - 1), N, K, K, B * T, int(w4)))
    v = _rows_view(x, K)
    if v is None:
        return False
    M, lda, _ = v
    return bool(_lib.mixdq_qlinear_f16in_supported(M, N, K, lda, M, int(w4)))


def qlinear_f16in_wanted(x: torch.Tensor, N: int, K: int, *, w4: bool = False, bos: bool = False,
                         w2: bool = False, abits: int = 8) -> bool:
    """What the modules ask: fuse this layer's quantize into its GEMM?  Supported, and -- under the default
    MIXDQ_F16IN=auto -- expected to be cheaper than the two launches (mixdq_qlinear_f16in_preferred)."""
    if F16IN == "0" or not qlinear_f16in_supported(x, N, K, w4=w4, bos=bos, w2=w2, abits=abits):
        return False
    if F16IN == "1":
        return True
    M = x.size(0) * (x.size(1) - 1) if bos else x.numel() // K
    return bool(_lib.mixdq_qlinear_f16in_preferred(M, N, K, int(w4)))


def qlinear_f16in(input_f16, scale_inv, zero_point, weight_int8, scale, bias0, bias=None, *,
                  _out=None, _bos=False, _cfg=0, _residual=None, _residual_div=1, _w4=False, _trace=None,
                  _w2=False):
    """quantize_per_tensor_to_int8(input, scale_inv, zero_point) -> qlinear_w8_a8_ohalf(...) in ONE launch
    (bit-identical to the pair).  `input_f16`: fp16 [..., K] readable in place as rows a constant stride
    apart; `_bos`: input is [B, T, K] and tokens 1.. are the operand, written to rows 1.. of `_out`
    [B, T, N] (QuantizedLinear's BOS path).  Raises where qlinear_f16in_supported() is False.
    `_trace`: the PERSISTENT tensor the weight operand is a view of (a 1x1 conv hands over a fresh
    permute / reshape view of its buffer on every call: the prefetch planner keeps weak references, and a
    reference to a temporary is dead on the next forward -- ADVICE r5)."""
    _trace_w(weight_int8 if _trace is None else _trace)
    _check(input_f16.is_cuda and input_f16.dtype == torch.float16, "input should be fp16 on GPU")
    dev = input_f16.device
    for t, nm in ((scale_inv, "scale_inv"), (zero_point, "zero_point"), (weight_int8, "weight_int8"),
                  (scale, "scale"), (bias0, "bias0")):
        _check(t.device == dev, f"input and {nm} should be on the same device.")
    _check(scale_inv.dtype == torch.float32 and zero_point.dtype == torch.float32,
           "scale_inv and zero_point should be fp32")
    _check(weight_int8.dtype == torch.int8, "weight_int8 should be int8 type")
    _check(scale.dtype == torch.float32 and bias0.dtype == torch.float32,
           "scale and bias0 should be float32")
    wflag = _wflag(_w4, _w2)
    N, K = weight_int8.size(0), weight_int8.size(1) * _kmul(_w4, _w2)
    _check(scale.numel() == N and bias0.numel() == N,
           "The size of scale and bias0 should be equal to output_channels.")
    if bias is not None:
        _check(bias.dtype == torch.float16 and bias.numel() == N and bias.device == dev,
               "bias should be fp16 of output_channels on the input's device")
    _check(input_f16.size(-1) == K,
           f"The last dimension of input and weight should match, got {input_f16.size(-1)} and {K}.")
    if _bos:
        _check(input_f16.dim() == 3 and input_f16.is_contiguous() and input_f16.size(1) >= 2,
               "BOS input should be a contiguous [B, T, K] tensor with T >= 2")
        B, T = input_f16.size(0), input_f16.size(1)
        M, lda, rm, flags = B * (T - 1), K, (T - 1, T, 1), FLAG_A_ROWMAP
        D = _out if _out is not None else torch.empty((B, T, N), dtype=torch.float16, device=dev)
    else:
        v = _rows_view(input_f16, K)
        _check(v is not None, "input rows should be a constant stride apart")
        M, lda, lead = v
        rm, flags = (0, 0, 0), 0
        D = _out if _out is not None else torch.empty(lead + [N], dtype=torch.float16, device=dev)
    w = weight_int8.contiguous()
    sc, b0 = _f32vec(scale), _f32vec(bias0)
    bs = None if bias is None else bias.contiguous()
    if _residual is not None:
        _check(_residual.dtype == torch.float16 and _residual.is_contiguous()
               and _residual.numel() == (M // _residual_div) * N,
               "residual should be contiguous fp16 of M / residual_div rows")
    _record("linear_f16in", M, N, K, K, _w4, qlinear_f16in,
            (input_f16, scale_inv, zero_point, weight_int8, scale, bias0, bias),
            dict(_out=_out, _bos=_bos, _cfg=_cfg, _residual=_residual, _residual_div=_residual_div,
                 _w4=_w4, _w2=_w2), w2=_w2)
    with torch.cuda.device(dev):
        code = _lib.mixdq_qlinear_f16in_w8a8(
            input_f16.data_ptr(), lda, scale_inv.data_ptr(), zero_point.data_ptr(), w.data_ptr(),
            b0.data_ptr(), sc.data_ptr(), _ptr(bs), D.data_ptr(), M, N, K, rm[0], rm[1], rm[2],
            _ptr(_residual), _residual_div,
            FLAGS | flags | (_cfg << 8) | wflag, _stream())
    _status(code, "qlinear_f16in")
    return D


_lib.mixdq_qlinear_w8a8_grouped.argtypes = [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_qlinear_w8a8_grouped.restype = _i32


class GemmGroupTable:
    """Device array of `mixdq_gemm_group` members (include/mixdq_hip.h) for qlinear_grouped.
    members: iterable of (weight_int8 [N, K], bias0 [N], scale [N], bias fp16 [N] or None,
    out fp16 tensor whose data_ptr() is the member's output base).  The table keeps references to
    every tensor it points at; `key` identifies the storage it was built for.  `wbits`: how every
    member's weight is stored -- 8 (int8), 4 (packed W4, [N, K/2]) or 2 (packed W2, [N, K/4]);
    `w4=True` is the older spelling of wbits=4."""

    def __init__(self, members, w4=False, wbits=None):
        import numpy as np
        self.members = [tuple(m) for m in members]
        if wbits is None:
            wbits = 4 if w4 else 8
        _check(wbits in (8, 4, 2) and not (w4 and wbits != 4), "wbits: 8, 4 or 2")
        self.wbits = int(wbits)
        self.w4 = self.wbits == 4
        self.w2 = self.wbits == 2
        rows, keep = [], []
        for w, b0, sc, bias, out in self.members:
            _check(w.is_cuda and w.dtype == torch.int8 and w.is_contiguous(), "member weight: int8")
            N = w.size(0)
            b0, sc = _f32vec(b0), _f32vec(sc)
            bias = None if bias is None else bias.contiguous()
            _check(b0.numel() == N and sc.numel() == N and (bias is None or bias.numel() == N),
                   "member epilogue vectors should have N elements")
            # the kernel cannot validate a device-side table: row stride == the member's N, whole
            # 8-byte output quads, 16-byte aligned operands
            _check(out.dtype == torch.float16 and out.data_ptr() % 16 == 0 and out.is_contiguous()
                   and out.dim() >= 1 and out.shape[-1] == N and N > 0 and out.numel() % N == 0,
                   "member output: contiguous fp16 [..., N], 16-byte aligned")
            _check(N % 4 == 0, "Int8 kernel with input or output alignment not to 4 is not supported.")
            _check(w.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 8 == 0)
                   and (bias is None or bias.dtype == torch.float16),
                   "member weight / bias: 16- / 8-byte aligned, bias fp16")
            keep.append((w, b0, sc, bias, out))
            rows.append([w.data_ptr(), b0.data_ptr(), sc.data_ptr(),
                         0 if bias is None else bias.data_ptr(), out.data_ptr(), N])
        self._keep = keep
        self.K = self.members[0][0].size(1) * (8 // self.wbits)
        _check(all(m[0].size(1) == self.members[0][0].size(1) for m in self.members),
               "members of a grouped launch share K")
        self.max_N = max(r[5] for r in rows)
        self.n = len(rows)
        # struct mixdq_gemm_group: 5 pointers, int32 N, int32 reserved = 6 x 8 bytes
        self.table = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.members[0][0].device)
        self.key = tuple(r[0] for r in rows) + tuple(r[4] for r in rows)


def qlinear_grouped(input_int8, table: "GemmGroupTable", *, _row_map=None, _cfg=0):
    """`table.n` Linears on the same int8 input in one launch (mixdq_qlinear_w8a8_grouped); every
    member writes its own output tensor (the ones the table was built with)."""
    _check(input_int8.is_cuda and input_int8.dtype == torch.int8, "input_int8 should be int8 on GPU")
    _check(input_int8.size(-1) == table.K, "The last dimension of input and weight should match")
    a = input_int8.contiguous()
    M = a.numel() // table.K if table.K else 0
    rm = _row_map or (0, 0, 0)
    _record("linear_grouped", M, sum(m[0].size(0) for m in table.members), table.K, table.K,
            table.w4, qlinear_grouped,
            (input_int8, table), dict(_row_map=_row_map, _cfg=_cfg), w2=table.w2)
    with torch.cuda.device(a.device):
        code = _lib.mixdq_qlinear_w8a8_grouped(a.data_ptr(), table.table.data_ptr(), table.n, M,
                                               table.max_N, table.K, rm[0], rm[1], rm[2],
                                               FLAGS | (_cfg << 8) | _wflag(table.w4, table.w2),
                                               _stream())
    _status(code, "qlinear_grouped")


_lib.mixdq_qlinear_w8a8_attn.argtypes = [_vp] * 7 + [_i64, _i32, _i32, _i32, _i32, _i64, _i32, _i64,
                                          _i32, ctypes.c_float, _vp, _vp, _i32, _vp]
_lib.mixdq_qlinear_w8a8_attn.restype = _i32


def qlinear_attention_supported(x_shape, N, K, k) -> bool:
    """Shapes the fused to_q + cross-attention launch takes (see qlinear_attention)."""
    return (len(x_shape) == 3 and N % 128 == 0 and K % 128 == 0 and x_shape[1] % 64 == 0
            and k.dim() == 3 and 0 < k.shape[1] <= 128 and k.shape[2] == N
            and x_shape[0] * x_shape[1] * K < 2 ** 32 and N * K < 2 ** 32)


def qlinear_attention(input_int8, weight_int8, scale, bias0, k, v, scale_inv=None, zero_point=None,
                      softmax_scale=None, *, _w4=False, _w2=False, _abits=8):
    """attn2.to_q (INT8 GEMM, no bias) and the cross-attention core in one launch
    (mixdq_qlinear_w8a8_attn): input int8 [B, T, K], weight [N, K], k / v fp16 [B, Tkv <= 128, N]
    with unit stride along N.  Returns the attention output [B, T, N]: int8 (to_out.0's operand)
    when scale_inv / zero_point are given, else fp16.  Bit-identical to qlinear_w8_a8_ohalf
    followed by attention_f16.  `_abits=4`: to_out.0's quantizer is a 4-bit one."""
    _trace_w(weight_int8)
    _check(input_int8.is_cuda and input_int8.dtype == torch.int8 and input_int8.dim() == 3,
           "input_int8 should be an int8 [B, T, K] GPU tensor")
    _check(weight_int8.dtype == torch.int8, "weight_int8 should be int8 type")
    wflag = _wflag(_w4, _w2)
    N, K = weight_int8.size(0), weight_int8.size(1) * _kmul(_w4, _w2)
    B, T, _ = input_int8.shape
    _check(input_int8.size(-1) == K, "The last dimension of input and weight should match")
    for t, n in ((k, "k"), (v, "v")):
        _check(t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.stride(-1) == 1
               and t.shape[0] == B and t.shape[2] == N, f"{n} should be fp16 [B, Tkv, N]")
    _check(k.shape == v.shape, "k / v shapes disagree")
    _check(qlinear_attention_supported(input_int8.shape, N, K, k),
           "qlinear_attention: unsupported configuration (N % 128, K % 128, T % 64, Tkv <= 128)")
    quant = scale_inv is not None
    a, w = input_int8.contiguous(), weight_int8.contiguous()
    out = torch.empty((B, T, N), dtype=torch.int8 if quant else torch.float16, device=a.device)
    sc, b0 = _f32vec(scale), _f32vec(bias0)
    ss = float(softmax_scale) if softmax_scale is not None else 0.125
    _record("linear_attn", B * T, N, K, K, _w4, qlinear_attention,
            (input_int8, weight_int8, scale, bias0, k, v, scale_inv, zero_point, softmax_scale),
            dict(_w4=_w4, _w2=_w2, _abits=_abits), w2=_w2)
    with torch.cuda.device(a.device):
        code = _lib.mixdq_qlinear_w8a8_attn(
            a.data_ptr(), w.data_ptr(), b0.data_ptr(), sc.data_ptr(), k.data_ptr(), v.data_ptr(),
            out.data_ptr(), B * T, N, K, T, k.shape[1], k.stride(0), k.stride(1), v.stride(0),
            v.stride(1), ss, _ptr(scale_inv), _ptr(zero_point),
            FLAGS | wflag | _aflag(_abits), _stream())
    _status(code, "qlinear_attention")
    return out


_lib.mixdq_qlinear_w8a8_geglu.argtypes = [_vp] * 6 + [_i64, _i32, _i32, _vp, _vp, _i32, _vp]
_lib.mixdq_qlinear_w8a8_geglu.restype = _i32


GELU_TABLE_MAG = 0x4c00   # csrc/igemm.hip kGeluTabMag: the table covers |gate| < 16


def silu_table(device="cuda"):
    """(table [n_pos + n_neg] uint16 as int16 tensor, n_pos, n_neg): the FP16 -> FP16 SiLU table of the GroupNorm apply
    pass's large-launch variant (mixdq_silu_table); building it eagerly keeps the init kernel out of captured graphs."""
    _lib.mixdq_silu_table.argtypes = [_vp, _vp, _vp, _vp]
    _lib.mixdq_silu_table.restype = _i32
    n_pos, n_neg = ctypes.c_int(0), ctypes.c_int(0)
    with torch.cuda.device(device):
        _status(_lib.mixdq_silu_table(None, ctypes.byref(n_pos), ctypes.byref(n_neg), _stream()), "silu_table")
        out = torch.empty(n_pos.value + n_neg.value, dtype=torch.int16, device=device)
        _status(_lib.mixdq_silu_table(out.data_ptr(), None, None, _stream()), "silu_table")
    return out, n_pos.value, n_neg.value


def gelu_table(device="cuda") -> torch.Tensor:
    """The table the GEMM + GEGLU epilogue of the large tiles looks GELU up in (mixdq_gelu_table):
    int16 [2, 0x4c00] -- row 0: gates +0 .. +16, row 1: -0 .. -16 -- of f16 bit patterns."""
    _lib.mixdq_gelu_table.argtypes = [_vp, _vp]
    _lib.mixdq_gelu_table.restype = _i32
    out = torch.empty((2, GELU_TABLE_MAG), dtype=torch.int16, device=device)
    with torch.cuda.device(out.device):
        _status(_lib.mixdq_gelu_table(out.data_ptr(), _stream()), "gelu_table")
    return out


def geglu_row_order(D: int, device=None) -> torch.Tensor:
    """Row order of mixdq_qlinear_w8a8_geglu's weight: value|gate groups of 16.  perm[i] = the row
    of the ordinary [2D, K] GEGLU projection (values 0..D-1, gates D..2D-1) stored at row i."""
    g = torch.arange(D // 16, device=device)[:, None] * 16 + torch.arange(16, device=device)[None, :]
    return torch.stack([g, g + D], dim=1).reshape(-1)


def qlinear_geglu(input_int8, weight_int8, scale, bias0, bias, out_scale_inv, out_zero_point, *,
                  _cfg=0, _w4=False, _out=None, _w2=False):
    """int8 [..., K] x value/gate-interleaved W [2D, K] -> int8 [..., D]: ff.net.0.proj + GEGLU +
    the quantizer of ff.net.2 in one launch (include/mixdq_hip.h: mixdq_qlinear_w8a8_geglu).
    `_out`: a contiguous int8 tensor of the result's size to write into (8-byte aligned)."""
    _trace_w(weight_int8)
    _check(input_int8.is_cuda and input_int8.dtype == torch.int8, "input_int8 should be int8 on GPU")
    _check(weight_int8.dtype == torch.int8, "weight_int8 should be int8 type")
    wflag = _wflag(_w4, _w2)
    N, K = weight_int8.size(0), weight_int8.size(1) * _kmul(_w4, _w2)
    _check(input_int8.size(-1) == K, "The last dimension of input and weight should match")
    _check(scale.numel() == N and bias0.numel() == N, "scale and bias0 should have 2D elements")
    a, w = input_int8.contiguous(), weight_int8.contiguous()
    M = a.numel() // K if K else 0
    out = _out if _out is not None else torch.empty(list(input_int8.shape[:-1]) + [N // 2],
                                                    dtype=torch.int8, device=a.device)
    _check(out.dtype == torch.int8 and out.is_contiguous() and out.numel() == M * (N // 2),
           "_out should be a contiguous int8 tensor of the result's size")
    sc, b0 = _f32vec(scale), _f32vec(bias0)
    bs = None if bias is None else bias.contiguous()
    _record("linear_geglu", M, N, K, K, _w4, qlinear_geglu,
            (input_int8, weight_int8, scale, bias0, bias, out_scale_inv, out_zero_point),
            dict(_cfg=_cfg, _w4=_w4, _w2=_w2), w2=_w2)
    with torch.cuda.device(a.device):
        code = _lib.mixdq_qlinear_w8a8_geglu(a.data_ptr(), w.data_ptr(), b0.data_ptr(),
                                             sc.data_ptr(), _ptr(bs), out.data_ptr(), M, N, K,
                                             _ptr(out_scale_inv), _ptr(out_zero_point),
                                             FLAGS | (_cfg << 8) | wflag,
                                             _stream())
    _status(code, "qlinear_geglu")
    return out


if hasattr(_lib, "mixdq_conv_halo_select"):      # (absent in older builds used for A/B runs)
    _lib.mixdq_conv_halo_select.argtypes = [_i32] * 9
    _lib.mixdq_conv_halo_select.restype = _i32
if hasattr(_lib, "mixdq_conv_halo_select_flags"):
    _lib.mixdq_conv_halo_select_flags.argtypes = [_i32] * 10
    _lib.mixdq_conv_halo_select_flags.restype = _i32


def conv_halo_select(N, H, W, C, K, R, S, stride, padding, w4=False) -> int:
    """Tile id (HALO_TILES key) of the LDS-resident-halo kernel an unforced INT8 conv of this shape
    runs on, or 0 (the implicit-GEMM family).  w4: for packed 4-bit weights (the kernel's W4
    instantiations; 0 in a library without them, or with MIXDQ_HALO_W4=0)."""
    if w4:
        if not hasattr(_lib, "mixdq_conv_halo_select_flags"):
            return 0
        return int(_lib.mixdq_conv_halo_select_flags(N, H, W, C, K, R, S, stride, padding, FLAG_W4))
    if not hasattr(_lib, "mixdq_conv_halo_select"):
        return 0
    return int(_lib.mixdq_conv_halo_select(N, H, W, C, K, R, S, stride, padding))


def _conv_geometry(input_int8, weight_int8, stride, padding, dilation):
    N, C, H, W = input_int8.shape
    K, _, R, S = weight_int8.shape
    P = (H + 2 * padding - dilation * (R - 1) - 1) // stride + 1
    Q = (W + 2 * padding - dilation * (S - 1) - 1) // stride + 1
    return N, C, H, W, K, R, S, P, Q


def conv_upsample2x_supported(x_shape, weight_shape, stride, padding, w4=False) -> bool:
    """qconv2d_w8_a8_ohalf(..., _upsample2x=True) takes this conv (the LDS-halo kernel's range).
    weight_shape: [K, C, R, S] of the unpacked weights; w4: they are stored packed."""
    N, C, H, W = x_shape
    K, _, R, S = weight_shape
    return conv_halo_select(N, 2 * H, 2 * W, C, K, R, S, stride, padding, w4) != 0


def qconv2d_w8_a8_ohalf(input_int8, weight_int8, weight_scale, input_scale, input_zero_point,
                        scale, weight_sum_by_input_channels, bias0, bias=None, stride=1,
                        padding=0, dilation=1, *, _table=None, _cfg=0, _residual=None,
                        _residual_per_image=False, _w4=False, _upsample2x=False):
    _trace_w(weight_int8)
    stride = 1 if stride is None else int(stride)
    padding = 0 if padding is None else int(padding)
    dilation = 1 if dilation is None else int(dilation)
    _check(input_int8.is_cuda, "Input should be on GPU.")
    dev = input_int8.device
    _check(dev == weight_int8.device, "input and weight_int8 should be on the same device.")
    _check(dev == weight_scale.device, "input and weight_scale should be on the same device.")
    _check(dev == input_scale.device, "input and input_scale should be on the same device.")
    _check(dev == input_zero_point.device,
           "input and input_zero_point should be on the same device.")
    wsum = weight_sum_by_input_channels
    if wsum is not None:
        _check(dev == wsum.device,
               "input and weight_sum_by_input_channels should be on the same device.")
    if bias0 is not None:
        _check(dev == bias0.device, "input and bias0 should be on the same device.")
    if bias is not None:
        _check(dev == bias.device, "input and bias should be on the same device.")
    _check(input_int8.dtype == torch.int8, "input_int8 should be int8 type")
    _check(weight_int8.dtype == torch.int8, "weight_int8 should be int8 type")
    _check(weight_scale.dtype == torch.float32,
           "Currently only support weight_scale with float32 type")
    _check(input_scale.dtype == torch.float32,
           "Currently only support input_scale with float32 type")
    _check(input_zero_point.dtype == torch.float32,
           "Currently only support input_zero_point with float32 type")
    if wsum is not None:
        _check(wsum.dtype == torch.float32,
               "Currently only support weight_sum_by_input_channels with float32 type")
    if bias0 is not None:
        _check(bias0.dtype == torch.float32, "Currently only support bias0 with float32 type")
    if bias is not None:
        _check(bias.dtype == torch.float16, "Currently only support bias with float16 type")
    _check(scale.dtype == torch.float32, "scale should be float32")
    _check(input_int8.dim() == 4 and weight_int8.dim() == 4, "input and weight should be 4-D")
    N, C, H, W, K, R, S, P, Q = _conv_geometry(input_int8, weight_int8, stride, padding, dilation)
    if _upsample2x:       # the conv runs on the nearest 2x upsampling of the stored input
        H, W = 2 * H, 2 * W
        P = (H + 2 * padding - (R - 1) - 1) // stride + 1
        Q = (W + 2 * padding - (S - 1) - 1) // stride + 1
    _check(weight_int8.size(1) * (2 if _w4 else 1) == C,
           "input and weight channel counts should match")
    _check(weight_scale.numel() == K,
           "The size of the weight_scale vector should be equal to output_channels.")
    if padding == 0:
        _check(bias0 is not None and bias0.numel() == K,
               "The size of bias0 should equal output_channels.")
    else:
        _check(wsum is not None and wsum.numel() == K * R * S,
               "The size of weight_sum_by_input_channels should equal K*R*S.")
    if bias is not None:
        _check(bias.numel() == K,
               "The size of the bias vector should be equal to output_channels.")
    x = input_int8.contiguous(memory_format=torch.channels_last)
    w = weight_int8.contiguous(memory_format=torch.channels_last)
    D = torch.empty((N, K, P, Q), dtype=torch.float16, device=dev,
                    memory_format=torch.channels_last)
    sc = _f32vec(scale)
    bs = None if bias is None else bias.contiguous()
    kind = "conv"
    if RECORD is not None and _cfg in (0, 90, 91, 92, 93) and dilation == 1:
        tile = _cfg or conv_halo_select(N, H, W, C, K, R, S, stride, padding, _w4)
        kind = f"conv_halo{tile}" if tile else "conv"
    _record(kind, N * P * Q, K, R * S * C, C, _w4, qconv2d_w8_a8_ohalf,
            (input_int8, weight_int8, weight_scale, input_scale, input_zero_point, scale,
             weight_sum_by_input_channels, bias0, bias, stride, padding, dilation),
            dict(_table=_table, _cfg=_cfg, _residual=_residual,
                 _residual_per_image=_residual_per_image, _w4=_w4, _upsample2x=_upsample2x))
    with torch.cuda.device(dev):
        res_ptr, res_div = None, 1
        if _residual is not None:
            _check(_residual.dtype == torch.float16, "residual should be fp16")
            if _residual_per_image:       # [N, K] (or [N, K, 1, 1]) row per image
                _check(_residual.is_contiguous() and _residual.numel() == N * K,
                       "per-image residual should be contiguous [N, K]")
                res_div = P * Q
            else:                         # [N, K, P, Q] channels-last
                _check(tuple(_residual.shape) == (N, K, P, Q) and _residual.is_contiguous(
                    memory_format=torch.channels_last), "residual should be channels-last [N,K,P,Q]")
            res_ptr = _residual.data_ptr()
        if padding > 0 and _table is None and _residual is None and not _upsample2x:
            ws_bytes = _lib.mixdq_qconv2d_workspace_bytes(K, R, S, padding)
            workspace = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
            code = _lib.mixdq_qconv2d_w8a8(
                x.data_ptr(), w.data_ptr(), sc.data_ptr(), wsum.contiguous().data_ptr(),
                input_zero_point.data_ptr(), None, _ptr(bs), D.data_ptr(), workspace.data_ptr(),
                N, H, W, C, K, R, S, stride, padding, dilation,
                FLAGS | (_cfg << 8) | (FLAG_W4 if _w4 else 0), _stream())
        else:
            _check(dilation == 1, "qconv2d_w8_a8_ohalf: unsupported configuration "
                                  "(dilation must be 1)")
            if padding > 0 and _table is None:
                _table = conv_border_table(wsum)
            b0 = None if padding > 0 else _f32vec(bias0)
            code = _lib.mixdq_qconv2d_w8a8_table(
                x.data_ptr(), w.data_ptr(), sc.data_ptr(), _ptr(_table),
                input_zero_point.data_ptr(), _ptr(b0), _ptr(bs), D.data_ptr(),
                N, H, W, C, K, R, S, stride, padding, res_ptr, res_div,
                FLAGS | (_cfg << 8) | (FLAG_W4 if _w4 else 0)
                | (FLAG_UPSAMPLE2X if _upsample2x else 0), _stream())
    _status(code, "qconv2d_w8_a8_ohalf")
    return D


def conv_border_table(weight_sum_by_input_channels, out=None):
    """Tap-rectangle sums of wsum [K,1,R,S] -> [(R*R*S*S), K] f32 (include/mixdq_hip.h,
    mixdq_conv_border_table).  Depends only on the weights: QuantizedConv2d caches it (`out`: an
    existing table to rebuild in place)."""
    wsum = weight_sum_by_input_channels.contiguous()
    _check(wsum.is_cuda and wsum.dtype == torch.float32 and wsum.dim() == 4,
           "weight_sum_by_input_channels should be a float32 [K,1,R,S] GPU tensor")
    K, _, R, S = wsum.shape
    table = out
    if table is None:
        table = torch.empty((R * R * S * S, K), dtype=torch.float32, device=wsum.device)
    _check(tuple(table.shape) == (R * R * S * S, K) and table.dtype == torch.float32
           and table.is_contiguous() and table.device == wsum.device, "border table shape")
    with torch.cuda.device(wsum.device):
        code = _lib.mixdq_conv_border_table(wsum.data_ptr(), table.data_ptr(), K, R, S, _stream())
    _status(code, "conv_border_table")
    return table


def conv_zero_point_propagate(weight_sum_by_input_channels, input_zero_point, N, H, W, stride,
                              padding):
    """The reference's materialised bias0 [N,K,P,Q] f32 channels-last
    (conv_act_zero_point_propagate.cu:54-83); diagnostic, not on the fast path."""
    wsum = weight_sum_by_input_channels.contiguous()
    K, _, R, S = wsum.shape
    P = (H + 2 * padding - (R - 1) - 1) // stride + 1
    Q = (W + 2 * padding - (S - 1) - 1) // stride + 1
    out = torch.empty((N, K, P, Q), dtype=torch.float32, device=wsum.device,
                      memory_format=torch.channels_last)
    with torch.cuda.device(wsum.device):
        code = _lib.mixdq_conv_zero_point_propagate(
            wsum.data_ptr(), input_zero_point.data_ptr(), out.data_ptr(), N, H, W, K, R, S,
            stride, padding, _stream())
    _status(code, "conv_zero_point_propagate")
    return out


def qlinear_fp_reference(input, weight, bias=None):
    """FP16 debug GEMM: input [..., K] @ weight [K, N] (row-major, qlinear.cc:161).  `bias` is
    accepted and ignored, as in the reference (op/qlinear.py:92)."""
    _check(input.dtype == torch.float16, "input should be int8 type")      # sic, qlinear.cc:146
    _check(weight.dtype == torch.float16, "weight should be int8 type")    # sic, qlinear.cc:148
    _check(input.is_cuda and weight.is_cuda, "Input should be on GPU.")
    if bias is not None:
        _check(input.device == bias.device, "input and bias should be on the same device.")
        _check(bias.dtype == torch.float16, "Currently only support bias with float16 type")
    K, N = weight.size(0), weight.size(1)
    a = input.contiguous()
    b = weight.contiguous()
    M = a.numel() // K if K else 0
    D = torch.empty(list(input.shape[:-1]) + [N], dtype=torch.float16, device=input.device)
    with torch.cuda.device(input.device):
        code = _lib.mixdq_gemm_f16(a.data_ptr(), b.data_ptr(), D.data_ptr(), M, N, K, _stream())
    _status(code, "qlinear_fp_reference")
    return D


# ---------------------------------------------------------------------------------------------
# FP16 layers (include/mixdq_hip.h: mixdq_linear_f16 / mixdq_conv2d_f16): the reference's FP fallback
# (F.linear / F.conv2d on the FP16 weight) on this repo's own MFMA kernels.
# ---------------------------------------------------------------------------------------------
_lib.mixdq_linear_f16.argtypes = [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp]
_lib.mixdq_linear_f16.restype = _i32
_lib.mixdq_conv2d_f16.argtypes = [_vp] * 4 + [_i32] * 9 + [_vp, _i64, _i32, _vp]
_lib.mixdq_conv2d_f16.restype = _i32


def linear_f16(input, weight, bias=None, *, _residual=None, _cfg=0, _act=None):
    """F.linear(input, weight, bias) for fp16 GPU tensors: input [..., K], weight [N, K] -> [..., N],
    FP32 accumulation, bias added in FP32, one rounding to fp16; `_residual` (fp16, the output's
    shape) is added after that rounding as a following torch half add would.
    `_act`: None, "gelu" (erf form) or "quick_gelu" (x * sigmoid(1.702 x)) -- the activation applied in the
    epilogue to that rounded fp16 value, rounded to fp16 again: what the stock activation behind a stock FP16 Linear
    computes (include/mixdq_math.h mixdq_geluf / mixdq_quick_geluf).  Not together with `_residual`."""
    _check(_act in FLAG_ACT, f"_act should be None, 'gelu' or 'quick_gelu', got {_act!r}")
    _trace_w(weight)
    _check(input.is_cuda and input.dtype == torch.float16, "input should be an fp16 GPU tensor")
    _check(weight.dtype == torch.float16 and weight.device == input.device and weight.dim() == 2,
           "weight should be an fp16 [N, K] tensor on the input's device")
    N, K = weight.shape
    _check(input.size(-1) == K, "The last dimension of input and weight should match")
    if bias is not None:
        _check(bias.dtype == torch.float16 and bias.numel() == N, "bias should be fp16 [N]")
    a, w = input.contiguous(), weight.contiguous()
    M = a.numel() // K if K else 0
    D = torch.empty(list(input.shape[:-1]) + [N], dtype=torch.float16, device=a.device)
    if _residual is not None:
        _check(_residual.dtype == torch.float16 and _residual.is_contiguous()
               and _residual.numel() == M * N, "residual should be contiguous fp16 [M, N]")
    bs = None if bias is None else bias.contiguous()
    with torch.cuda.device(a.device):
        code = _lib.mixdq_linear_f16(a.data_ptr(), w.data_ptr(), _ptr(bs), D.data_ptr(), M, N, K,
                                     _ptr(_residual), 1, (int(_cfg) << 8) | FLAG_ACT[_act], _stream())
    _status(code, "linear_f16")
    return D


def conv2d_f16(input, weight, bias=None, stride=1, padding=0, *, _residual=None,
               _residual_per_image=False, _cfg=0, _upsample2x=False, _pad_after=False):
    """F.conv2d(input, weight, bias, stride, padding) for fp16 GPU tensors (square stride / padding,
    dilation 1, groups 1): input [N, C, H, W] and weight [K, C, R, S] are read in channels-last
    memory (converted if they are not), the result is channels-last [N, K, P, Q].
    `_upsample2x`: the conv runs on F.interpolate(input, scale_factor=2, mode="nearest") without that tensor being
    made (MIXDQ_FLAG_UPSAMPLE2X: 3x3 / stride 1 / padding 1 on the MFMA tiles -- C % 8 == 0, K % 4 == 0 -- only;
    anything else is refused); same bits as the conv on the materialised tensor.
    `_pad_after`: the `padding` rows and columns of zeros lie below and right of the image only
    (MIXDQ_FLAG_PAD_AFTER): F.conv2d(F.pad(input, (0, padding, 0, padding)), weight, bias, stride, 0) without the padded
    tensor, same bits; 3x3 / stride 2 / padding 1 is the conv of diffusers' Downsample2D in a VAE encoder.  On the
    MFMA tiles and the one-output-per-thread kernel alike; not together with `_upsample2x`."""
    _trace_w(weight)
    _check(input.is_cuda and input.dtype == torch.float16 and input.dim() == 4,
           "input should be a 4-D fp16 GPU tensor")
    _check(weight.dtype == torch.float16 and weight.device == input.device and weight.dim() == 4,
           "weight should be a 4-D fp16 tensor on the input's device")
    stride, padding = int(stride), int(padding)
    N, C, H, W, K, R, S, P, Q = _conv_geometry(input, weight, stride, padding, 1)
    if _upsample2x:       # the conv runs on the nearest 2x upsampling of the stored input
        H, W = 2 * H, 2 * W
        P = (H + 2 * padding - (R - 1) - 1) // stride + 1
        Q = (W + 2 * padding - (S - 1) - 1) // stride + 1
    if _pad_after:        # zeros below and right only (with _upsample2x: the library refuses the pair)
        P = max((H + padding - R) // stride + 1, 0)
        Q = max((W + padding - S) // stride + 1, 0)
    _check(weight.size(1) == C, "input and weight channel counts should match")
    if bias is not None:
        _check(bias.dtype == torch.float16 and bias.numel() == K, "bias should be fp16 [K]")
    x = input.contiguous(memory_format=torch.channels_last)
    w = weight.contiguous(memory_format=torch.channels_last)
    D = torch.empty((N, K, P, Q), dtype=torch.float16, device=x.device,
                    memory_format=torch.channels_last)
    res_ptr, res_div = None, 1
    if _residual is not None:
        _check(_residual.dtype == torch.float16, "residual should be fp16")
        if _residual_per_image:
            _check(_residual.is_contiguous() and _residual.numel() == N * K,
                   "per-image residual should be contiguous [N, K]")
            res_div = P * Q
        else:
            _check(tuple(_residual.shape) == (N, K, P, Q) and _residual.is_contiguous(
                memory_format=torch.channels_last), "residual should be channels-last [N,K,P,Q]")
        res_ptr = _residual.data_ptr()
    bs = None if bias is None else bias.contiguous()
    with torch.cuda.device(x.device):
        code = _lib.mixdq_conv2d_f16(x.data_ptr(), w.data_ptr(), _ptr(bs), D.data_ptr(), N, H, W, C,
                                     K, R, S, stride, padding, res_ptr, res_div,
                                     (int(_cfg) << 8) | (FLAG_UPSAMPLE2X if _upsample2x else 0)
                                     | (FLAG_PAD_AFTER if _pad_after else 0), _stream())
    _status(code, "conv2d_f16")
    return D


# ---------------------------------------------------------------------------------------------
# Producer fusions (include/mixdq_hip.h, csrc/fused_norm.hip).  Not part of the reference's `_C`:
# used by mixdq_amd.unet's fused forward.  Same no-fallback rule: GPU tensors only.
# ---------------------------------------------------------------------------------------------
_lib.mixdq_groupnorm_workspace_bytes.restype = _sz
_lib.mixdq_groupnorm_workspace_bytes.argtypes = [_i32, _i64, _i32, _i32]
_lib.mixdq_groupnorm_silu_quantize.restype = _i32
_lib.mixdq_groupnorm_silu_quantize.argtypes = [_vp, _vp, _vp, ctypes.c_float, _i32, _vp, _vp, _vp,
                                               _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp]
_lib.mixdq_groupnorm_silu_quantize2.restype = _i32
_lib.mixdq_groupnorm_silu_quantize2.argtypes = [_vp, _i32, _vp, _vp, _vp, ctypes.c_float, _i32, _vp,
                                                _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _vp]
_lib.mixdq_groupnorm_silu_quantize3.restype = _i32
_lib.mixdq_groupnorm_silu_quantize3.argtypes = [_vp, _i32, _vp, _vp, _vp, ctypes.c_float, _i32, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32,
                                                _i32, _i32, _vp]
_lib.mixdq_layernorm_quantize.restype = _i32
_lib.mixdq_layernorm_quantize.argtypes = [_vp, _vp, _vp, ctypes.c_float, _i64, _i32, _i32, _vp, _vp,
                                          _vp, _vp, _i32, _vp]
_lib.mixdq_geglu_quantize.restype = _i32
_lib.mixdq_geglu_quantize.argtypes = [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp]


def groupnorm_supported(N, HW, C, G) -> bool:
    return _lib.mixdq_groupnorm_workspace_bytes(N, HW, C, G) > 0


def groupnorm_workspace(N, HW, C, num_groups, device) -> torch.Tensor:
    """A workspace for groupnorm_silu_quantize launches of this shape (`_workspace=`): owned by the caller, one
    launch at a time per buffer."""
    ws_bytes = _lib.mixdq_groupnorm_workspace_bytes(int(N), int(HW), int(C), int(num_groups))
    _check(ws_bytes > 0, "groupnorm_silu_quantize: unsupported configuration")
    return torch.empty(ws_bytes // 4, dtype=torch.float32, device=device)


def groupnorm_silu_quantize(x, num_groups, weight, bias, eps, scale_inv=None, zero_point=None,
                            silu=True, want_f16=False, x2=None, raw_qparams=None, *, _workspace=None):
    """x: fp16 [N, C, H, W] in channels-last memory (or [N, HW, C] contiguous).  Returns
    (int8 or None, fp16 or None) with x's shape and strides.
    x2 (same layout, same N / H / W): the GroupNorm of cat([x, x2], dim=channels) without making
    the concatenation; the outputs have the concatenated shape.
    raw_qparams: one (scale_inv, zero_point) pair or None per source tensor; the return value gains
    a third element, the list of `quantize_per_tensor(source)` results (None where not asked for),
    written by the same pass."""
    _check(x.is_cuda and x.dtype == torch.float16, "x should be an fp16 GPU tensor")
    if x.dim() == 4:
        _check(x.is_contiguous(memory_format=torch.channels_last),
               "groupnorm_silu_quantize needs channels-last input")
        N, C, HW = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    else:
        _check(x.dim() == 3 and x.is_contiguous(), "x should be [N, HW, C] contiguous")
        N, HW, C = x.shape
    C1 = C
    shape = tuple(x.shape)
    if x2 is not None:
        _check(x2.is_cuda and x2.dtype == torch.float16 and x2.dim() == x.dim()
               and x2.shape[0] == N and (x2.shape[2:] == x.shape[2:] if x.dim() == 4
                                         else x2.shape[1] == HW)
               and (x2.is_contiguous(memory_format=torch.channels_last) if x.dim() == 4
                    else x2.is_contiguous()), "x2 should match x in batch / spatial size and layout")
        C2 = x2.shape[1] if x.dim() == 4 else x2.shape[2]
        _check(C1 % 8 == 0 and C2 % 8 == 0, "two-source GroupNorm needs channel counts % 8 == 0")
        C = C1 + C2
        shape = (N, C, x.shape[2], x.shape[3]) if x.dim() == 4 else (N, HW, C)
    fmt = dict(memory_format=torch.channels_last) if x.dim() == 4 else {}
    want_q = scale_inv is not None
    _check(want_q or want_f16, "nothing to compute")
    ws_bytes = _lib.mixdq_groupnorm_workspace_bytes(N, HW, C, num_groups)
    _check(ws_bytes > 0, "groupnorm_silu_quantize: unsupported configuration")
    if _workspace is not None:
        _check(_workspace.device == x.device and _workspace.numel() * _workspace.element_size() >= ws_bytes,
               "groupnorm_silu_quantize: workspace too small (groupnorm_workspace)")
        ws = _workspace
    else:
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    out_q = torch.empty(shape, dtype=torch.int8, device=x.device, **fmt) if want_q else None
    out_h = torch.empty(shape, dtype=torch.float16, device=x.device, **fmt) if want_f16 else None
    w, b = weight.contiguous(), bias.contiguous()
    _check(w.dtype == torch.float16 and b.dtype == torch.float16, "gamma/beta should be fp16")
    raws = None
    arr = ctypes.c_void_p * 2
    r_si = r_zp = r_q = None
    if raw_qparams is not None:
        sources = [x] if x2 is None else [x, x2]
        _check(len(raw_qparams) == len(sources), "one raw quantizer slot per source tensor")
        raws = [None if qp is None else torch.empty_like(src, dtype=torch.int8)
                for qp, src in zip(raw_qparams, sources)]
        pad = [None] * (2 - len(sources))
        r_si = arr(*[_ptr(None if qp is None else qp[0]) for qp in list(raw_qparams) + pad])
        r_zp = arr(*[_ptr(None if qp is None else qp[1]) for qp in list(raw_qparams) + pad])
        r_q = arr(*[_ptr(t) for t in raws + pad])
    with torch.cuda.device(x.device):
        code = _lib.mixdq_groupnorm_silu_quantize3(
            x.data_ptr(), C1, _ptr(x2), w.data_ptr(), b.data_ptr(), float(eps),
            int(bool(silu)), _ptr(scale_inv), _ptr(zero_point), _ptr(out_q), _ptr(out_h),
            r_si, r_zp, r_q, ws.data_ptr(), N, HW, C, num_groups, FLAGS, _stream())
    _status(code, "groupnorm_silu_quantize")
    if raw_qparams is not None:
        return out_q, out_h, raws
    return out_q, out_h


def layernorm_quantize(x, weight, bias, eps, qparams, want_f16=False, *, _abits=None):
    """x: fp16 [..., C] contiguous; qparams: up to three (scale_inv, zero_point) device-scalar
    pairs.  Returns ([int8 ...], fp16 or None).  `_abits`: the width of each quantizer, e.g. (8, 4, 8)
    (default: all 8)."""
    _check(x.is_cuda and x.dtype == torch.float16 and x.is_contiguous(),
           "x should be a contiguous fp16 GPU tensor")
    C = x.shape[-1]
    M = x.numel() // C if C else 0
    n = len(qparams)
    _check(n <= 3 and (n > 0 or want_f16), "layernorm_quantize: 1..3 quantizers or want_f16")
    abits = (8,) * n if _abits is None else tuple(_abits)
    _check(len(abits) == n, "layernorm_quantize: one width per quantizer")
    aflags = 0
    for i, b in enumerate(abits):
        aflags |= _aflag(b, i)
    outs = [torch.empty_like(x, dtype=torch.int8) for _ in range(n)]
    out_h = torch.empty_like(x) if want_f16 else None
    arr = ctypes.c_void_p * max(n, 1)
    si = arr(*[p[0].data_ptr() for p in qparams])
    zp = arr(*[p[1].data_ptr() for p in qparams])
    oq = arr(*[o.data_ptr() for o in outs])
    w, b = weight.contiguous(), bias.contiguous()
    _check(w.dtype == torch.float16 and b.dtype == torch.float16, "gamma/beta should be fp16")
    with torch.cuda.device(x.device):
        code = _lib.mixdq_layernorm_quantize(x.data_ptr(), w.data_ptr(), b.data_ptr(), float(eps),
                                             M, C, n, si, zp, oq, _ptr(out_h), FLAGS | aflags, _stream())
    _status(code, "layernorm_quantize")
    return outs, out_h


_lib.mixdq_qlinear_ln_workspace_bytes.restype = _sz
_lib.mixdq_qlinear_ln_workspace_bytes.argtypes = [_i64, _i32]
_lib.mixdq_qlinear_ln_select_id.restype = _i32
_lib.mixdq_qlinear_ln_select_id.argtypes = [_i64, _i32, _i32]
_lib.mixdq_qlinear_w8a8_ln.restype = _i32
_lib.mixdq_qlinear_w8a8_ln.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp,
                                       ctypes.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]

# GEMM + residual + LayerNorm + quantize in one launch (csrc/igemm_ln.hip).  MIXDQ_LN_FUSE=0: off (A/B runs).
LN_FUSE = os.environ.get("MIXDQ_LN_FUSE", "1") != "0"


def qlinear_ln_supported(M: int, N: int, K: int) -> bool:
    return bool(LN_FUSE and _lib.mixdq_qlinear_ln_select_id(int(M), int(N), int(K)) > 0)


def qlinear_ln_workspace(M: int, N: int, device) -> torch.Tensor:
    """A zeroed exchange buffer for qlinear_ln launches of up to M rows x N columns: its first page holds the
    launch counter (the epoch: it only grows -- every launch tags its records with epoch + 1), the departure
    counter (zero between launches) and a sticky error word (qlinear_ln_status); the records follow.  Owned by
    the caller: one launch at a time per buffer AND per device (the tiles of a launch wait for each other)."""
    return torch.zeros(int(_lib.mixdq_qlinear_ln_workspace_bytes(int(M), int(N))), dtype=torch.uint8,
                       device=device)


_lib.mixdq_qlinear_ln_status.restype = _i32
_lib.mixdq_qlinear_ln_status.argtypes = [_vp, _vp, _vp]


def qlinear_ln_status(workspace) -> int:
    """The workspace's sticky error word: 0 while every launch on it found all its records, else the tag of the
    last launch in which a workgroup gave up waiting (its rows were written as NaN).  Synchronises the stream."""
    w = ctypes.c_int(0)
    with torch.cuda.device(workspace.device):
        code = _lib.mixdq_qlinear_ln_status(workspace.data_ptr(), ctypes.byref(w), _stream())
    _status(code, "qlinear_ln_status")
    return int(w.value)


def qlinear_ln(input_int8, weight_int8, scale, bias0, bias, residual, ln_weight, ln_bias, eps, qparams,
               workspace, *, want_f16=False, _cfg=0):
    """y = qlinear_w8_a8_ohalf(input_int8, ...) [+ residual];  layernorm_quantize(y, ln_weight, ln_bias, eps,
    qparams, want_f16) -- in ONE launch, bit-identical to the two (mixdq_qlinear_w8a8_ln).  Returns
    (y fp16 [..., N], [int8 ...], fp16 or None).  Raises where qlinear_ln_supported() is False."""
    _trace_w(weight_int8)
    _check(input_int8.is_cuda and input_int8.dtype == torch.int8, "input_int8 should be int8 on GPU")
    dev = input_int8.device
    N, K = weight_int8.size(0), weight_int8.size(1)
    _check(input_int8.size(-1) == K, "The last dimension of input and weight should match")
    a, w = input_int8.contiguous(), weight_int8.contiguous()
    M = a.numel() // K if K else 0
    lead = list(input_int8.shape[:-1])
    D = torch.empty(lead + [N], dtype=torch.float16, device=dev)
    n = len(qparams)
    _check(n <= 3 and (n > 0 or want_f16), "qlinear_ln: 1..3 quantizers or want_f16")
    outs = [torch.empty(lead + [N], dtype=torch.int8, device=dev) for _ in range(n)]
    out_h = torch.empty(lead + [N], dtype=torch.float16, device=dev) if want_f16 else None
    arr = ctypes.c_void_p * max(n, 1)
    si = arr(*[p[0].data_ptr() for p in qparams])
    zp = arr(*[p[1].data_ptr() for p in qparams])
    oq = arr(*[o.data_ptr() for o in outs])
    sc, b0 = _f32vec(scale), _f32vec(bias0)
    bs = None if bias is None else bias.contiguous()
    g, b = ln_weight.contiguous(), ln_bias.contiguous()
    _check(g.dtype == torch.float16 and b.dtype == torch.float16 and g.numel() == N and b.numel() == N,
           "LayerNorm weight / bias should be fp16 [N]")
    if residual is not None:
        _check(residual.dtype == torch.float16 and residual.is_contiguous() and residual.numel() == M * N,
               "residual should be contiguous fp16 [M, N]")
    _check(workspace.is_cuda and workspace.device == dev and workspace.numel() >=
           _lib.mixdq_qlinear_ln_workspace_bytes(M, N), "workspace too small (qlinear_ln_workspace)")
    _record("linear_ln", M, N, K, K, False, qlinear_ln,
            (input_int8, weight_int8, scale, bias0, bias, residual, ln_weight, ln_bias, eps, qparams, workspace),
            dict(want_f16=want_f16, _cfg=_cfg))
    with torch.cuda.device(dev):
        code = _lib.mixdq_qlinear_w8a8_ln(a.data_ptr(), w.data_ptr(), b0.data_ptr(), sc.data_ptr(), _ptr(bs),
                                          D.data_ptr(), M, N, K, _ptr(residual), 1, g.data_ptr(), b.data_ptr(),
                                          float(eps), n, si, zp, oq, _ptr(out_h), workspace.data_ptr(),
                                          FLAGS | (_cfg << 8), _stream())
    _status(code, "qlinear_ln")
    return D, outs, out_h


def geglu_quantize(h, scale_inv=None, zero_point=None, want_f16=False, *, _abits=8):
    """h: fp16 [..., 2D] contiguous -> (int8 [..., D] or None, fp16 [..., D] or None).
    `_abits=4`: the output quantizer is a 4-bit one."""
    _check(h.is_cuda and h.dtype == torch.float16 and h.is_contiguous(),
           "h should be a contiguous fp16 GPU tensor")
    D = h.shape[-1] // 2
    M = h.numel() // (2 * D) if D else 0
    want_q = scale_inv is not None
    _check(want_q or want_f16, "nothing to compute")
    shape = list(h.shape[:-1]) + [D]
    out_q = torch.empty(shape, dtype=torch.int8, device=h.device) if want_q else None
    out_h = torch.empty(shape, dtype=torch.float16, device=h.device) if want_f16 else None
    with torch.cuda.device(h.device):
        code = _lib.mixdq_geglu_quantize(h.data_ptr(), M, D, _ptr(scale_inv), _ptr(zero_point),
                                         _ptr(out_q), _ptr(out_h), FLAGS | _aflag(_abits), _stream())
    _status(code, "geglu_quantize")
    return out_q, out_h


_lib.mixdq_attention_f16.argtypes = [_vp] * 4 + [_i32] * 5 + [_i64] * 8 + [ctypes.c_float, _vp, _vp,
                                                                       _i32, _vp]
_lib.mixdq_attention_f16.restype = _i32


if hasattr(_lib, "mixdq_attention_f16_prefetch"):     # (absent in older builds used for A/B runs)
    _lib.mixdq_attention_f16_prefetch.argtypes = [_vp] * 4 + [_i32] * 5 + [_i64] * 8 + [
        ctypes.c_float, _vp, _vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), _i32, _i32, _vp]
    _lib.mixdq_attention_f16_prefetch.restype = _i32
PREFETCH_MAX_RANGES = 16


# head widths of mixdq_attention_f16 (64: the SDXL kernels; 40, 80, 160: SD 1.5's, csrc/attention.hip attn_hd_kernel;
# 512: the VAE decoder's single head, attn_512_kernel -- FP16 output only)
ATTENTION_HEAD_DIMS = (40, 64, 80, 160, 512)


def attention_f16(q, k, v, heads, scale_inv=None, zero_point=None, softmax_scale=None, _cfg=0, _prefetch=None,
                  _abits=8, _causal=False):
    """FP16 attention core (the reference's get_attention_scores + bmm, quant_block.py:630-637).

    q [B, Tq, C], k/v [B, Tkv, C] fp16 with unit stride along C (column slices of a fused projection
    are read in place); C = heads * D, head width D in ATTENTION_HEAD_DIMS (64: SDXL; 40, 80, 160: SD 1.5; 512: the
    VAE decoder -- FP16 output only: with `scale_inv` the library answers MIXDQ_ERR_SHAPE, as it does to `_cfg != 0`).
    `softmax_scale` defaults to D ** -0.5.  Returns fp16 [B, Tq, C], or — when `scale_inv`/`zero_point`
    (to_out.0's activation quantizer) are given — its int8 quantization.
    `_prefetch`: up to 16 GPU tensors (the weights of the layers behind this attention) that payload
    workgroups of the launch read while the attention runs (mixdq_attention_f16_prefetch); no effect
    on the result.
    `_abits=4`: to_out.0's quantizer is a 4-bit one (the INT8 output clamped to [-128, -113]).
    `_cfg`: 0 = the library's choice; 4 / 2 = 128- / 64-query workgroups of the tiled kernel; 1 = the short-key
    kernel (Tkv <= 128: every key of a head staged once), at every head width -- what `_cfg=0` picks for so few
    keys (MIXDQ_ATTN_SHORT=0 at width 64, MIXDQ_ATTN_HD_SHORT=0 at 40 / 80 / 160 keep the tiled kernel: A/B runs).
    `_cfg=1` with more keys is refused (MIXDQ_ERR_SHAPE).  Every form gives the same bits.
    `_causal=True`: query row i attends to keys 0 .. i (MIXDQ_FLAG_CAUSAL: a text encoder's self-attention) -- head
    width 64, Tq == Tkv <= 128, FP16 output, `_cfg` 0 or 1; anything else is refused (MIXDQ_ERR_SHAPE).
    """
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _check(t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.stride(-1) == 1,
               f"{n} should be a [B, T, C] fp16 GPU tensor with unit stride along C")
    B, Tq, C = q.shape
    _check(k.shape == v.shape and k.shape[0] == B and k.shape[2] == C, "q/k/v shapes disagree")
    D = C // heads if heads > 0 else 0
    _check(C == heads * D and D in ATTENTION_HEAD_DIMS, "head_dim must be 64, 40, 80, 160 or 512")
    quant = scale_inv is not None
    # (measurement only) recorded as ("attention", (B * heads * Tq, Tkv, D, D)): 4 * M * N * K FLOPs
    _record("attention", B * heads * Tq, k.shape[1], D, D, False, attention_f16,
            (q, k, v, heads), dict(scale_inv=scale_inv, zero_point=zero_point,
                                   softmax_scale=softmax_scale, _cfg=_cfg, _abits=_abits,
                                   _causal=_causal))     # (measured without the payload)
    out = torch.empty((B, Tq, C), dtype=torch.int8 if quant else torch.float16, device=q.device)
    sc = float(softmax_scale) if softmax_scale is not None else (0.125 if D == 64 else D ** -0.5)
    ctx = getattr(_TLS, "ctx", None)
    # a launch that can carry a payload (head_dim 64 only: the other widths' kernel ignores one)
    if D == 64 and k.shape[1] > 128 and ctx is not None and ctx.device == q.device:
        ctx.trace.append(("attn", B * Tq, k.shape[1]))
        planned = ctx.payload()
        if _prefetch is None:
            _prefetch = planned
    # (a payload address of another device would be dereferenced by this device's kernel: dropped)
    pf = [t for t in (_prefetch or ()) if t is not None and t.device == q.device and t.numel() > 0]
    _check(len(pf) <= PREFETCH_MAX_RANGES, "at most 16 prefetch ranges")
    with torch.cuda.device(q.device):
        if pf and hasattr(_lib, "mixdq_attention_f16_prefetch"):
            ptrs = (ctypes.c_void_p * len(pf))(*[t.data_ptr() for t in pf])
            sizes = (ctypes.c_int64 * len(pf))(*[t.numel() * t.element_size() for t in pf])
            code = _lib.mixdq_attention_f16_prefetch(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, heads, D, Tq, k.shape[1],
                q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                out.stride(0), out.stride(1), sc, _ptr(scale_inv), _ptr(zero_point), ptrs, sizes, len(pf),
                FLAGS | (int(_cfg) << 8) | _aflag(_abits) | (FLAG_CAUSAL if _causal else 0), _stream())
        else:
            code = _lib.mixdq_attention_f16(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, heads, D, Tq, k.shape[1],
                q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                out.stride(0), out.stride(1), sc, _ptr(scale_inv), _ptr(zero_point),
                FLAGS | (int(_cfg) << 8) | _aflag(_abits) | (FLAG_CAUSAL if _causal else 0), _stream())
    _status(code, "attention_f16")
    return out


_lib.mixdq_embed_tokens_f16.argtypes = [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_embed_tokens_f16.restype = _i32


def embed_tokens_f16(ids, tok, pos):
    """Token + position embedding of a text encoder (mixdq_embed_tokens_f16):
    out[b, t, :] = fp16(fp32(tok[ids[b, t]]) + fp32(pos[t])).

    ids: int32 [B, T] GPU tensor; tok: fp16 [V, C]; pos: fp16 [Tmax, C] with T <= Tmax; C % 8 == 0.  Returns fp16
    [B, T, C].  An id outside [0, V) is clamped into the range (a negative id reads row 0, an id >= V row V - 1):
    the kernel cannot report an error, and this layer does not read the ids back to check them -- that would wait
    for the GPU and break a graph capture."""
    _check(ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous(),
           "ids should be a contiguous int32 [B, T] GPU tensor")
    for t_, n in ((tok, "tok"), (pos, "pos")):
        _check(t_.dtype == torch.float16 and t_.device == ids.device and t_.dim() == 2 and t_.is_contiguous(),
               f"{n} should be a contiguous fp16 2-D tensor on the ids' device")
    B, T = ids.shape
    V, C = tok.shape
    _check(pos.shape[1] == C and T <= pos.shape[0], "pos should be [Tmax, C] with T <= Tmax")
    _check(V >= 1 and C % 8 == 0, "tok should be [V >= 1, C] with C % 8 == 0")
    out = torch.empty((B, T, C), dtype=torch.float16, device=ids.device)
    with torch.cuda.device(ids.device):
        code = _lib.mixdq_embed_tokens_f16(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, C, V,
                                           _stream())
    _status(code, "embed_tokens_f16")
    return out


# The eight step entry points (include/mixdq_hip.h): the names of their arguments in order, the trailing stream aside.
# The argument types are read off the names here, and _sampler_step assembles every call from them.
_STEP_SHARED = " timestep guidance n rows_per_image row_stride"
_STEP_MASKED = " z noise0 mask channels blend"
_STEP_FLAT = "x eps inp table width t_table n_steps step timestep guidance image_guidance "   # (the two flat ones)
_STEP_ARGS = {
    "": "x eps inp noise noise_stride table t_table n_steps step" + _STEP_SHARED,
    "_rng": "x eps inp seeds n_image table t_table n_steps step" + _STEP_SHARED,
    "_2m": "x eps inp hist table t_table n_steps step first" + _STEP_SHARED,
    "3": _STEP_FLAT + "n row_stride noise noise_stride seeds n_image hist first" + _STEP_MASKED,
    "_rescaled": _STEP_FLAT + ("rescale rows_per_image n n_image row_stride workspace noise noise_stride seeds hist first"
                               + _STEP_MASKED)}
_STEP_ARGS.update({"_masked": _STEP_ARGS[""] + _STEP_MASKED, "_masked_rng": _STEP_ARGS["_rng"] + _STEP_MASKED,
                   "_2m_masked": _STEP_ARGS["_2m"] + _STEP_MASKED})
_STEP_CTYPES = {**dict.fromkeys(("n", "n_image", "row_stride", "noise_stride"), _i64),
                **dict.fromkeys(("width", "n_steps", "rows_per_image", "channels"), _i32),
                **dict.fromkeys(("guidance", "image_guidance", "rescale"), ctypes.c_float)}   # everything else: a pointer
for _name, _args in _STEP_ARGS.items():
    getattr(_lib, "mixdq_sampler_step" + _name).argtypes = [_STEP_CTYPES.get(a, _vp) for a in _args.split()] + [_vp]
    getattr(_lib, "mixdq_sampler_step" + _name).restype = _i32
_lib.mixdq_sampler_rescale_workspace_floats.argtypes = [_i64, _i64]
_lib.mixdq_sampler_rescale_workspace_floats.restype = ctypes.c_size_t
_lib.mixdq_randn_f32.argtypes = [_vp, _i32, _i64, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp]
_lib.mixdq_randn_f32.restype = _i32
_lib.mixdq_rng_normals_from_bits.argtypes = [_vp, _vp, _i64, _vp]
_lib.mixdq_rng_normals_from_bits.restype = _i32
RNG_STREAM_START, RNG_STREAM_STEP, RNG_STREAM_VAE = 0, 1, 2               # include/mixdq_hip.h MIXDQ_RNG_STREAM_*
RNG_STREAM_COND = 3                                                       # ... the blanked image's posterior (9-channel UNets)


def _check_seeds(seeds, B, what):
    _check(torch.is_tensor(seeds) and seeds.dtype == torch.int64 and seeds.dim() == 1 and seeds.shape[0] == B
           and seeds.is_contiguous(), f"{what}: seeds should be a contiguous int64 tensor of shape [{B}]")


def randn(shape, seeds, stream=0, step=0, out=None):
    """Standard normals made on the device (mixdq_randn_f32): fp32 [B, C, H, W] in channels-last storage.  seeds: int64
    GPU tensor [B], one per image, its bits read as unsigned.  Element e = (h * W + w) * C + c of image b is lane e & 3
    of Philox4x32-10 with key seeds[b] and counter (e >> 2, step, stream) through Box-Muller (include/mixdq_math.h):
    an image's values depend on its seed and shape only.  stream: RNG_STREAM_START (0), _STEP (1, with `step` the index
    of the sampler step that adds it), _VAE (2), _COND (3).  out: a dense channels-last fp32 tensor of that shape to fill."""
    _check(len(shape) == 4 and all(int(d) >= 1 for d in shape[1:]) and int(shape[0]) >= 0,
           "randn: shape should be (B, C, H, W)")
    B, C, H, W = (int(d) for d in shape)
    _check_seeds(seeds, B, "randn")
    _check(seeds.is_cuda, "randn: seeds should be on the GPU")
    _check(0 <= int(stream) < 2 ** 32 and 0 <= int(step) < 2 ** 32, "randn: stream and step are unsigned 32-bit values")
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=seeds.device).permute(0, 3, 1, 2)
    else:
        _check(torch.is_tensor(out) and out.dtype == torch.float32 and out.device == seeds.device
               and tuple(out.shape) == (B, C, H, W) and out.permute(0, 2, 3, 1).is_contiguous(),
               "randn: out should be a dense channels-last fp32 tensor of the shape on the seeds' device")
    with torch.cuda.device(seeds.device):
        code = _lib.mixdq_randn_f32(out.data_ptr(), B, C * H * W, seeds.data_ptr(), int(stream), int(step), _stream())
    _status(code, "randn")
    return out


def rng_normals_from_bits(r):
    """Test hook (mixdq_rng_normals_from_bits): int32 GPU tensor [n, 4] -- the raw 32-bit words, their bits read as
    unsigned -- -> fp32 [n, 4]."""
    _check(torch.is_tensor(r) and r.is_cuda and r.dtype == torch.int32 and r.dim() == 2 and r.shape[1] == 4
           and r.is_contiguous(), "rng_normals_from_bits: r should be a contiguous int32 [n, 4] GPU tensor")
    z = torch.empty(r.shape, dtype=torch.float32, device=r.device)
    with torch.cuda.device(r.device):
        code = _lib.mixdq_rng_normals_from_bits(r.data_ptr(), z.data_ptr(), r.shape[0], _stream())
    _status(code, "rng_normals_from_bits")
    return z


def _sampler_step(what, x, eps, inp, table, width, t_table, step, timestep, guidance, rows_per_image, n, row_stride, *,
                  hist=None, first=None, masked=None, channels=4, noise=None, noise_stride=None, seeds=None,
                  n_image=None, image_guidance=None, rescale=None, workspace=None):
    """The checks and the call of the step bindings.  `what`: the binding's name; `table`: coef (width 4) or, for
    the multistep kinds, coef8 (width 8), which come with `hist` and `first`; masked: None or (z, noise0, mask, blend);
    noise / seeds: at most one of them, width 4 only; image_guidance: None, or the second scale of the three-row step
    (mixdq_sampler_step3, rows_per_image == 3); rescale: None, or phi of the rescaled step
    (mixdq_sampler_step_rescaled, rows_per_image 2 or 3), which comes with `workspace` and `n_image`."""
    # n and n_image, once.  The checks of `seeds=` / `n_image=` come first and look at no device, so that a wrong call
    # is refused the same way wherever it is made.
    _check(seeds is None or noise is None,
           f"{what}: noise and seeds exclude each other (with seeds the step makes its own noise)")
    n = int((x.numel() if torch.is_tensor(x) else 0) if n is None else n)
    if seeds is not None or rescale is not None:      # the modes that know of images
        n_image = n if n_image is None else int(n_image)
        _check(n_image >= 1 and n % n_image == 0, f"{what}: n = {n} is not a multiple of n_image = {n_image}")
    if seeds is not None:
        _check_seeds(seeds, n // n_image, what)
    f32, f16, i32 = torch.float32, torch.float16, torch.int32
    two_m = width == 8
    tname = "coef8" if two_m else "coef"
    z, noise0, mask, blend = masked if masked is not None else (None,) * 4
    operands = [(x, "x", f32), (eps, "eps", f16), (inp, "inp", f16)] + [(hist, "hist", f32)] * two_m + [
        (table, tname, f32), (t_table, "t_table", f32), (step, "step", i32)] + [(first, "first", i32)] * two_m + [
        (timestep, "timestep", f32)]
    if masked is not None:
        operands += [(z, "z", f32), (noise0, "noise0", f32), (mask, "mask", f32), (blend, "blend", f32)]
    if noise is not None:
        operands.append((noise, "noise", f32))
    if seeds is not None:
        operands.append((seeds, "seeds", torch.int64))
    if rescale is not None:
        operands.append((workspace, "workspace", f32))
    for t_, name, dt in operands:
        _check(torch.is_tensor(t_) and t_.is_cuda and t_.device == x.device and t_.dtype == dt,
               f"{name} should be a {dt} tensor on x's GPU")
    _check(table.dim() == 2 and table.shape[1] == width and table.is_contiguous() and t_table.is_contiguous(),
           f"{tname} should be a contiguous [n_steps, {width}] table")
    n_steps = table.shape[0]
    if masked is not None:
        _check(tuple(blend.shape) == (n_steps, 2) and blend.is_contiguous(),
               "blend should be a contiguous [n_steps, 2] table")
    _check(t_table.numel() >= n_steps + 1, "t_table needs n_steps + 1 entries")
    if two_m:
        _check(step.numel() == 1 and first.numel() == 1 and timestep.numel() == 1,
               "step, first and timestep hold one value each")
    else:
        _check(step.numel() == 1 and timestep.numel() == 1, "step and timestep hold one value each")
    row_stride = n if row_stride is None else int(row_stride)
    noise_stride = n if noise_stride is None else int(noise_stride)
    _check(0 <= n <= x.numel(), "n exceeds the state")
    if two_m:
        _check(hist.numel() >= n, "hist is smaller than the state")
    if masked is not None:
        channels = int(channels)
        _check(z.numel() >= n and noise0.numel() >= n, "z / noise0 are smaller than the state")
        if channels >= 1 and n % channels == 0:       # (anything else: the library's own error)
            _check(mask.is_contiguous() and mask.numel() >= n // channels,
                   "mask should be dense with n / channels entries")
    if rescale is not None:
        _check(workspace.is_contiguous() and workspace.numel() >= _lib.mixdq_sampler_rescale_workspace_floats(n, n_image),
               "workspace is smaller than sampler_rescale_workspace(n, n_image)")
    if rows_per_image in (1, 2) or image_guidance is not None:   # (anything else: the library's own error)
        need = (rows_per_image - 1) * row_stride + n
        _check(eps.numel() >= need and inp.numel() >= need, "eps / inp are smaller than rows_per_image row blocks")
    if noise is not None:
        _check(noise.numel() >= (n_steps - 1) * noise_stride + n, "noise is smaller than n_steps blocks")
    # the entry point, and its arguments by name (_STEP_ARGS); a flat one takes a mode's operands null where it is off
    entry = ("_rescaled" if rescale is not None else "3" if image_guidance is not None else
             ("_2m" if two_m else "") + ("_masked" if masked is not None else "") + ("_rng" if seeds is not None else ""))
    have = dict(x=x, eps=eps, inp=inp, table=table, width=width, t_table=t_table, n_steps=n_steps, step=step, first=first,
                timestep=timestep, guidance=float(guidance), image_guidance=float(image_guidance or 0.0), rescale=rescale,
                rows_per_image=int(rows_per_image), n=n, n_image=n_image or 0, row_stride=row_stride, workspace=workspace,
                noise=noise, noise_stride=noise_stride, seeds=seeds, hist=hist, z=z, noise0=noise0, mask=mask,
                channels=channels if masked is not None else 1, blend=blend)
    args = [_ptr(v) if v is None or torch.is_tensor(v) else v for v in map(have.get, _STEP_ARGS[entry].split())]
    with torch.cuda.device(x.device):
        code = getattr(_lib, "mixdq_sampler_step" + entry)(*args, _stream())
    _status(code, what)


def sampler_step(x, eps, inp, coef, t_table, step, timestep, guidance=0.0, rows_per_image=1, noise=None, *,
                 n=None, row_stride=None, noise_stride=None, seeds=None, n_image=None):
    """One sampler step in place (mixdq_sampler_step): guidance over the two row blocks of `eps`, the affine
    scheduler update of the FP32 state `x` with `coef[step]` = (a, b, c, s_next), the UNet's next FP16 input into
    every row block of `inp`; then `timestep` <- `t_table[step + 1]` and `step` += 1, on the device.

    x: fp32 state; eps / inp: fp16, `rows_per_image` blocks of `n` elements `row_stride` apart (unconditional block
    first); noise: None, or fp32 [n_steps] blocks `noise_stride` apart; coef: fp32 [n_steps, 4]; t_table: fp32
    [n_steps + 1]; step: int32 [1]; timestep: the fp32 0-dim tensor the UNet reads.  The kernel is elementwise over
    STORAGE: x, eps, inp and noise must be dense and share one stride pattern (the caller's business: Sampler checks
    it).  `n` defaults to x.numel(), the strides to n.

    seeds (int64 [n / n_image] on x's GPU, read as unsigned; `noise` must then be None): the step computes its noise in
    registers (mixdq_sampler_step_rng) -- the values randn(.., seeds, stream=RNG_STREAM_STEP, step=<step>) holds for
    images of `n_image` elements (default: n, one image)."""
    _sampler_step("sampler_step", x, eps, inp, coef, 4, t_table, step, timestep, guidance, rows_per_image, n, row_stride,
                  noise=noise, noise_stride=noise_stride, seeds=seeds, n_image=n_image)


def sampler_step_masked(x, eps, inp, coef, t_table, step, timestep, z, noise0, mask, blend, guidance=0.0,
                        rows_per_image=1, noise=None, *, channels=4, n=None, row_stride=None, noise_stride=None,
                        seeds=None, n_image=None):
    """sampler_step for inpainting (mixdq_sampler_step_masked): the same guidance and update, then the region the
    mask keeps is overwritten with the image latents at the next step's noise level,
    x = (1 - m) * (p * z + q * noise0) + m * x', (p, q) = blend[step], and the UNet's next input is taken from that.

    z, noise0: fp32, `n` elements in x's stride pattern; mask: fp32, one value per latent pixel ([B, h, w] dense,
    n / channels entries; 1 repaints, 0 keeps): element i of the channels-last storage belongs to entry
    i // channels; blend: fp32 [n_steps, 2] (Schedule.blend).  Everything else as sampler_step, `seeds` / `n_image`
    (mixdq_sampler_step_masked_rng) included."""
    _sampler_step("sampler_step_masked", x, eps, inp, coef, 4, t_table, step, timestep, guidance, rows_per_image, n,
                  row_stride, masked=(z, noise0, mask, blend), channels=channels, noise=noise,
                  noise_stride=noise_stride, seeds=seeds, n_image=n_image)


def sampler_step_2m(x, eps, inp, hist, coef8, t_table, step, first, timestep, guidance=0.0, rows_per_image=1, *,
                    n=None, row_stride=None):
    """One DPM-Solver++ 2M step in place (mixdq_sampler_step_2m): guidance as sampler_step, the data prediction
    x0 = u * x + v * e, a second-order update of `x` from x0 and `hist` (the previous step's x0) when `step` > `first`
    and the row's D2 != 0, a first-order one otherwise (hist is not read then); `hist` <- x0 on every step; the UNet's
    next FP16 input into every row block of `inp`; then `timestep` and `step` advance as in sampler_step.

    hist: fp32, `n` elements in x's stride pattern, not x itself; coef8: fp32 [n_steps, 8] (Schedule.coef of
    'dpmpp_2m'): (u, v, A, B1, B2, D2, s_next, 0); first: int32 [1], the index of the run's first step.  Everything
    else as sampler_step; there is no noise operand."""
    _sampler_step("sampler_step_2m", x, eps, inp, coef8, 8, t_table, step, timestep, guidance, rows_per_image, n,
                  row_stride, hist=hist, first=first)


def sampler_step_2m_masked(x, eps, inp, hist, coef8, t_table, step, first, timestep, z, noise0, mask, blend,
                           guidance=0.0, rows_per_image=1, *, channels=4, n=None, row_stride=None):
    """sampler_step_2m for inpainting (mixdq_sampler_step_2m_masked): the same step, then sampler_step_masked's blend
    of the new state with the image latents at the next step's noise level.  `hist` is the unblended x0.  z, noise0,
    mask, blend and channels as in sampler_step_masked."""
    _sampler_step("sampler_step_2m_masked", x, eps, inp, coef8, 8, t_table, step, timestep, guidance, rows_per_image, n,
                  row_stride, hist=hist, first=first, masked=(z, noise0, mask, blend), channels=channels)


def _check_flat(what, table, noise, seeds, hist, first, z, noise0, mask, blend):
    """The pre-checks of the two flat bindings, which take every mode's operands: the table's width says which kind the
    step is, and the operands of a mode go together.  Returns (width, masked) as _sampler_step takes them."""
    width = table.shape[1] if torch.is_tensor(table) and table.dim() == 2 else 4
    _check(width in (4, 8), f"{what}: table should be coef [n_steps, 4] or coef8 [n_steps, 8]")
    if width == 8:
        _check(noise is None and seeds is None, f"{what}: the multistep kinds add no noise")
        _check(hist is not None and first is not None, f"{what}: coef8 comes with hist and first")
    else:
        _check(hist is None and first is None, f"{what}: hist and first come with coef8")
    some = [t_ is not None for t_ in (z, noise0, mask, blend)]
    _check(all(some) or not any(some), f"{what}: z, noise0, mask and blend go together")
    return width, (z, noise0, mask, blend) if all(some) else None


def sampler_step3(x, eps, inp, table, t_table, step, timestep, guidance, image_guidance, *, noise=None, seeds=None,
                  n_image=None, hist=None, first=None, z=None, noise0=None, mask=None, blend=None, channels=4, n=None,
                  row_stride=None, noise_stride=None):
    """One sampler step with THREE UNet rows per image and two guidance scales (mixdq_sampler_step3; InstructPix2Pix).
    eps / inp: fp16, three blocks of `n` elements `row_stride` apart in diffusers' InstructPix2Pix order -- block 0 text +
    image (e_t), block 1 image only (e_i), block 2 neither (e_u); NOT the two-row convention, whose unconditional block
    comes first.  e = (e_u + guidance * (e_t - e_i)) + image_guidance * (e_i - e_u), then the sibling's step:

    table: coef fp32 [n_steps, 4] (sampler_step / sampler_step_masked, with `noise` or `seeds` / `n_image` as there), or
    coef8 fp32 [n_steps, 8] together with `hist` and `first` (sampler_step_2m[_masked]; no noise).  z, noise0, mask and
    blend (all four, with `channels`) add sampler_step_masked's blend.  The next FP16 input goes to all three blocks of
    `inp`; `timestep` and `step` advance as in sampler_step."""
    width, masked = _check_flat("sampler_step3", table, noise, seeds, hist, first, z, noise0, mask, blend)
    _sampler_step("sampler_step3", x, eps, inp, table, width, t_table, step, timestep, guidance, 3, n, row_stride,
                  hist=hist, first=first, masked=masked, channels=channels, noise=noise, noise_stride=noise_stride,
                  seeds=seeds, n_image=n_image, image_guidance=image_guidance)


def sampler_rescale_workspace(n, n_image, device):
    """The FP32 workspace sampler_step_rescaled needs for a state of `n` elements in images of `n_image`
    (mixdq_sampler_rescale_workspace_floats): per 2048-element chunk of an image four statistics, and one factor per
    image.  The caller keeps it (a Sampler: one static buffer); its contents need not survive between steps."""
    n, n_image = int(n), int(n_image)
    _check(n >= 0 and n_image >= 1 and n % n_image == 0, f"sampler_rescale_workspace: n = {n} is not a multiple of "
           f"n_image = {n_image}")
    return torch.zeros(max(int(_lib.mixdq_sampler_rescale_workspace_floats(n, n_image)), 4), dtype=torch.float32,
                       device=device)


def sampler_step_rescaled(x, eps, inp, table, t_table, step, timestep, guidance, image_guidance, rescale, workspace, *,
                          rows_per_image, n_image=None, noise=None, seeds=None, hist=None, first=None, z=None,
                          noise0=None, mask=None, blend=None, channels=4, n=None, row_stride=None, noise_stride=None):
    """One sampler step with guidance rescale (mixdq_sampler_step_rescaled; diffusers' guidance_rescale): the guided
    output of every image is multiplied by 1 + rescale * (std(t) / std(e) - 1) before the update -- t the
    text-conditioned output (rows_per_image 2: row block 1, sampler_step's order; 3: block 0, sampler_step3's order), e
    the guided one, the standard deviations over the image's `n_image` elements (default: n, one image).  Where a
    standard deviation is 0 the factor is 1 (diffusers: NaN).  rescale in [0, 1]; 0 is the plain step bit for bit.

    workspace: sampler_rescale_workspace(n, n_image, device).  image_guidance: the second scale of three rows, None
    (not read) with two.  Everything else -- table (coef, or coef8 with hist and first), noise or seeds, z / noise0 /
    mask / blend with channels -- as sampler_step3 takes it."""
    what = "sampler_step_rescaled"
    _check(rows_per_image in (2, 3), f"{what}: rows_per_image should be 2 or 3 (rescale compares the guided output "
           "with the text-conditioned one)")
    _check(isinstance(rescale, (int, float)) and 0.0 <= float(rescale) <= 1.0, f"{what}: rescale should be in [0, 1]")
    width, masked = _check_flat(what, table, noise, seeds, hist, first, z, noise0, mask, blend)
    _sampler_step(what, x, eps, inp, table, width, t_table, step, timestep, guidance, rows_per_image, n, row_stride,
                  hist=hist, first=first, masked=masked, channels=channels, noise=noise, noise_stride=noise_stride,
                  seeds=seeds, n_image=n_image, image_guidance=image_guidance if rows_per_image == 3 else None,
                  rescale=float(rescale), workspace=workspace)


_lib.mixdq_image_to_nhwc8_f16.argtypes = [_vp, _i32, _i64, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_image_to_nhwc8_f16.restype = _i32
_lib.mixdq_vae_latent_sample.argtypes = [_vp, _vp, _vp, _i64, _i32, ctypes.c_float, _vp]
_lib.mixdq_vae_latent_sample.restype = _i32
_lib.mixdq_image_to_nhwc8_f16_masked.argtypes = ([_vp, _i32] + [_i64] * 4 + [_vp, _i32] + [_i64] * 3
                                                 + [_vp, _i32, _i32, _i32, _i32, _vp])
_lib.mixdq_image_to_nhwc8_f16_masked.restype = _i32
_lib.mixdq_inpaint_cond_f16.argtypes = [_vp, _vp, _vp, _i64, _i32, _vp]
_lib.mixdq_inpaint_cond_f16.restype = _i32
_lib.mixdq_ip2p_cond_f16.argtypes = [_vp, _vp, _i32, _i64, _i32, _i32, ctypes.c_float, _vp]
_lib.mixdq_ip2p_cond_f16.restype = _i32
IMAGE_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}      # include/mixdq_hip.h MIXDQ_IMAGE_*


def image_to_nhwc8_f16(image, mask=None):
    """The VAE encoder's ingest (mixdq_image_to_nhwc8_f16): image [B, C <= 8, H, W], uint8, fp16 or fp32, of ANY
    strides (NCHW, channels-last, a slice: the kernel reads them) -> fp16 [B, 8, H, W] in channels-last storage,
    channels C..7 zero.  uint8: f16(f32(u) * f32(2/255) - 1), which is f16(u / 127.5 - 1); floats: f16(v), no clamp.
    `mask` ([B, H, W] or [B, 1, H, W] at the image's size, uint8 / fp16 / fp32 of any strides, set as in
    mask_to_latent): the pixels under it are stored as +0.0 in every channel (mixdq_image_to_nhwc8_f16_masked) --
    diffusers' init_image * (mask < 0.5), the "masked image" a 9-channel inpainting UNet is conditioned on."""
    _check(torch.is_tensor(image) and image.is_cuda and image.dim() == 4 and image.dtype in IMAGE_DTYPES,
           "image should be a 4-D uint8, fp16 or fp32 GPU tensor")
    B, C, H, W = image.shape
    _check(1 <= C <= 8, "image should have 1 to 8 channels")
    if mask is not None:
        mB, mH, mW, mst = _mask3(mask, "image_to_nhwc8_f16")
        _check(mask.device == image.device and (mB, mH, mW) == (B, H, W),
               "image_to_nhwc8_f16: mask should have the image's batch, height and width and be on its device")
    out = torch.empty((B, H, W, 8), dtype=torch.float16, device=image.device)
    sb, sc, sh, sw = image.stride()
    with torch.cuda.device(image.device):
        if mask is None:
            code = _lib.mixdq_image_to_nhwc8_f16(image.data_ptr(), IMAGE_DTYPES[image.dtype], sb, sc, sh, sw,
                                                 out.data_ptr(), B, C, H, W, _stream())
        else:
            code = _lib.mixdq_image_to_nhwc8_f16_masked(image.data_ptr(), IMAGE_DTYPES[image.dtype], sb, sc, sh, sw,
                                                        mask.data_ptr(), IMAGE_DTYPES[mask.dtype], *mst,
                                                        out.data_ptr(), B, C, H, W, _stream())
    _status(code, "image_to_nhwc8_f16")
    return out.permute(0, 3, 1, 2)


_lib.mixdq_control_chunk.restype = _i32
_lib.mixdq_control_add_f16.argtypes = [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp]
_lib.mixdq_control_add_f16.restype = _i32
_lib.mixdq_silu_f16.argtypes = [_vp, _vp, _i64, _vp]
_lib.mixdq_silu_f16.restype = _i32
_lib.mixdq_hint_to_nhwc8_f16.argtypes = [_vp, _i32, _i64, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_hint_to_nhwc8_f16.restype = _i32
CONTROL_CHUNK = _lib.mixdq_control_chunk()
CONTROL_MAX_SEGMENTS, CONTROL_MAX_NETS = 16, 4                            # include/mixdq_hip.h MIXDQ_CONTROL_MAX_*


def _dense_f16(t, what):
    """`t` is an fp16 GPU tensor whose elements occupy one dense run of memory (contiguous or channels-last)."""
    _check(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16, f"{what} should be an fp16 GPU tensor")
    _check(t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)),
           f"{what} should be dense (contiguous or channels-last)")


def _same_layout(a, b) -> bool:
    """Two dense tensors of one shape whose elements lie in memory in the same order."""
    if a.shape != b.shape:
        return False
    if a.is_contiguous() and b.is_contiguous():
        return True
    cl = torch.channels_last
    return a.dim() == 4 and a.is_contiguous(memory_format=cl) and b.is_contiguous(memory_format=cl)


def control_add(skips, residuals, scales, step, out=None):
    """Every skip tensor of a UNet plus the scaled residuals of K ControlNets, one launch (mixdq_control_add_f16).
    skips: S <= 16 fp16 tensors; residuals: K <= 4 lists of S fp16 tensors, residuals[k][i] of skips[i]'s shape AND
    strides (the operation is elementwise over storage); scales: fp32 [K, n_steps] on the device; step: the int32
    device tensor sampler_step* advances.  With c_k = scales[k, step]:
    out[i] = f16(skips[i] + (f16(r_0 * c_0) + f16(r_1 * c_1) + ...)), the sum left to right in fp16; a net whose c_k is 0
    is skipped and its residuals are not read; a step outside [0, n_steps) skips every net (out = skips).
    out: None (fresh tensors), or S tensors like the skips -- out[i] may be skips[i] itself.  Returns the list."""
    what = "control_add"
    _check(isinstance(skips, (list, tuple)) and 1 <= len(skips) <= CONTROL_MAX_SEGMENTS,
           f"{what}: skips should be a list of 1 to {CONTROL_MAX_SEGMENTS} tensors")
    _check(isinstance(residuals, (list, tuple)) and 1 <= len(residuals) <= CONTROL_MAX_NETS,
           f"{what}: residuals should be a list of 1 to {CONTROL_MAX_NETS} lists (one per net)")
    S, K = len(skips), len(residuals)
    dev = skips[0].device if torch.is_tensor(skips[0]) else None
    for i, s in enumerate(skips):
        _dense_f16(s, f"{what}: skips[{i}]")
        _check(s.device == dev, f"{what}: skips[{i}] is on another device")
        _check(s.numel() % 8 == 0 and s.data_ptr() % 16 == 0, f"{what}: skips[{i}] should have a multiple of 8 elements "
               "and be 16-byte aligned")
    for k, net in enumerate(residuals):
        _check(isinstance(net, (list, tuple)) and len(net) == S, f"{what}: residuals[{k}] should hold {S} tensors, one per "
               "skip")
        for i, r in enumerate(net):
            _dense_f16(r, f"{what}: residuals[{k}][{i}]")
            _check(r.device == dev and _same_layout(r, skips[i]),
                   f"{what}: residuals[{k}][{i}] should have the shape {tuple(skips[i].shape)}, the memory format and the "
                   f"device of skips[{i}], got {tuple(r.shape)}")
            _check(r.data_ptr() % 16 == 0, f"{what}: residuals[{k}][{i}] should be 16-byte aligned")
    _check(torch.is_tensor(scales) and scales.is_cuda and scales.device == dev and scales.dtype == torch.float32
           and scales.dim() == 2 and scales.shape[0] == K and scales.shape[1] >= 1 and scales.is_contiguous(),
           f"{what}: scales should be a contiguous fp32 [{K}, n_steps] tensor on the skips' device")
    _check(torch.is_tensor(step) and step.device == dev and step.dtype == torch.int32 and step.numel() == 1,
           f"{what}: step should be one int32 on the skips' device")
    if out is None:
        out = [torch.empty_like(s) for s in skips]       # (preserve_format: the skips' strides)
    else:
        _check(isinstance(out, (list, tuple)) and len(out) == S, f"{what}: out should hold {S} tensors")
        for i, o in enumerate(out):
            _dense_f16(o, f"{what}: out[{i}]")
            _check(o.device == dev and _same_layout(o, skips[i]) and o.data_ptr() % 16 == 0,
                   f"{what}: out[{i}] should be like skips[{i}]")
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])        # noqa: E731
    with torch.cuda.device(dev):
        code = _lib.mixdq_control_add_f16(ptrs(skips), ptrs(out), ptrs([r for net in residuals for r in net]),
                                          _i64arr([s.numel() for s in skips]), S, K, scales.data_ptr(), scales.shape[1],
                                          step.data_ptr(), _stream())
    _status(code, what)
    return list(out)


def silu_f16(x, out=None):
    """SiLU on a dense fp16 GPU tensor (mixdq_silu_f16): f16(x / (1 + exp(-x))) on the fp32 value of every element,
    include/mixdq_math.h mixdq_siluf.  out: None (a fresh tensor like x) or a tensor like x -- x itself runs in place."""
    _dense_f16(x, "silu_f16: x")
    _check(x.numel() % 8 == 0 and x.data_ptr() % 16 == 0, "silu_f16: x should have a multiple of 8 elements and be "
           "16-byte aligned")
    if out is None:
        out = torch.empty_like(x)
    else:
        _dense_f16(out, "silu_f16: out")
        _check(out.device == x.device and _same_layout(out, x) and out.data_ptr() % 16 == 0,
               "silu_f16: out should be like x")
    with torch.cuda.device(x.device):
        code = _lib.mixdq_silu_f16(x.data_ptr(), out.data_ptr(), x.numel(), _stream())
    _status(code, "silu_f16")
    return out


def hint_to_nhwc8_f16(image):
    """A ControlNet's image ingest (mixdq_hint_to_nhwc8_f16): image [B, C <= 8, H, W], uint8, fp16 or fp32, of ANY
    strides -> fp16 [B, 8, H, W] in channels-last storage, channels C..7 zero.  uint8: f16(f32(u) / 255), what
    image.float().div(255).half() gives; floats: f16(v), no clamp."""
    _check(torch.is_tensor(image) and image.is_cuda and image.dim() == 4 and image.dtype in IMAGE_DTYPES,
           "hint_to_nhwc8_f16: image should be a 4-D uint8, fp16 or fp32 GPU tensor")
    B, C, H, W = image.shape
    _check(1 <= C <= 8, "hint_to_nhwc8_f16: image should have 1 to 8 channels")
    out = torch.empty((B, H, W, 8), dtype=torch.float16, device=image.device)
    sb, sc, sh, sw = image.stride()
    with torch.cuda.device(image.device):
        code = _lib.mixdq_hint_to_nhwc8_f16(image.data_ptr(), IMAGE_DTYPES[image.dtype], sb, sc, sh, sw, out.data_ptr(),
                                            B, C, H, W, _stream())
    _status(code, "hint_to_nhwc8_f16")
    return out.permute(0, 3, 1, 2)


def vae_latent_sample(moments, noise=None, scaling_factor=1.0):
    """The posterior sample of an AutoencoderKL (mixdq_vae_latent_sample): moments fp16 [B, 2L, h, w] in
    channels-last storage (channels 0..L-1 the mean, L..2L-1 the log-variance), noise fp32 [B, L, h, w]
    channels-last or None -> fp32 [B, L, h, w] channels-last:
    (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scaling_factor; without noise mean * scaling_factor (the
    mode).  L % 4 == 0.  Arithmetic: include/mixdq_math.h mixdq_vae_latent."""
    _check(torch.is_tensor(moments) and moments.is_cuda and moments.dtype == torch.float16 and moments.dim() == 4
           and moments.shape[1] % 2 == 0 and moments.is_contiguous(memory_format=torch.channels_last),
           "moments should be a channels-last fp16 [B, 2L, h, w] GPU tensor")
    B, C2, h, w = moments.shape
    L = C2 // 2
    if noise is not None:
        _check(torch.is_tensor(noise) and noise.device == moments.device and noise.dtype == torch.float32
               and tuple(noise.shape) == (B, L, h, w) and noise.is_contiguous(memory_format=torch.channels_last),
               "noise should be a channels-last fp32 [B, L, h, w] tensor on the moments' device")
    z = torch.empty((B, h, w, L), dtype=torch.float32, device=moments.device)
    with torch.cuda.device(moments.device):
        code = _lib.mixdq_vae_latent_sample(moments.data_ptr(), _ptr(noise), z.data_ptr(), B * h * w, L,
                                            float(scaling_factor), _stream())
    _status(code, "vae_latent_sample")
    return z.permute(0, 3, 1, 2)


_lib.mixdq_mask_to_latent.argtypes = [_vp, _i32, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_mask_to_latent.restype = _i32
_lib.mixdq_composite_u8.argtypes = ([_vp] + [_i64] * 4) * 2 + [_vp, _i32] + [_i64] * 3 + [_vp, _i32, _i32, _i32, _vp]
_lib.mixdq_composite_u8.restype = _i32
MASK_MODES = {"nearest": 0, "any": 1}                                     # include/mixdq_hip.h MIXDQ_MASK_*


def _mask3(mask, what):
    """An image-resolution mask [B, H, W] or [B, 1, H, W] as (B, H, W, element strides)."""
    _check(torch.is_tensor(mask) and mask.is_cuda and mask.dtype in IMAGE_DTYPES
           and (mask.dim() == 3 or (mask.dim() == 4 and mask.shape[1] == 1)),
           f"{what}: mask should be a [B, H, W] or [B, 1, H, W] uint8, fp16 or fp32 GPU tensor")
    st = mask.stride()
    return mask.shape[0], mask.shape[-2], mask.shape[-1], (st[0], st[-2], st[-1])


def mask_to_latent(mask, mode="nearest"):
    """An image-resolution inpainting mask as the latent-resolution one Sampler.sample(mask=) takes
    (mixdq_mask_to_latent): mask [B, H, W] or [B, 1, H, W], uint8 (set: u >= 128), fp16 or fp32 (set: v >= 0.5; NaN is
    not set), of ANY strides, H and W multiples of 8 -> fp32 [B, H/8, W/8] of 0.0 / 1.0.  mode 'nearest': pixel
    (8i, 8j), what F.interpolate(mask, size=(H/8, W/8)) picks and so diffusers' pipeline; 'any': 1 where any pixel of
    the 8x8 block is set (a latent whose block touches the mask is repainted)."""
    _check(mode in MASK_MODES, f"mask_to_latent: mode should be one of {tuple(MASK_MODES)}")
    B, H, W, (sb, sh, sw) = _mask3(mask, "mask_to_latent")
    _check(H % 8 == 0 and W % 8 == 0, "mask_to_latent: H and W should be multiples of 8")
    out = torch.empty((B, H // 8, W // 8), dtype=torch.float32, device=mask.device)
    with torch.cuda.device(mask.device):
        code = _lib.mixdq_mask_to_latent(mask.data_ptr(), IMAGE_DTYPES[mask.dtype], sb, sh, sw, out.data_ptr(), B, H, W,
                                         MASK_MODES[mode], _stream())
    _status(code, "mask_to_latent")
    return out


def inpaint_cond(mask_lat, zl):
    """The conditioning channels of a 9-channel inpainting UNet (mixdq_inpaint_cond_f16): mask_lat fp32 [B, h, w] or
    [B, 1, h, w] dense (what mask_to_latent returns, or a soft mask: the values pass through), zl fp32 [B, L, h, w] in
    channels-last storage (what VAEEncoder.encode returns for the blanked image), 1 <= L <= 7 -> fp16 [B, 8, h, w] in
    channels-last storage: channel 0 f16(mask), channels 1..L f16(zl), the rest zero.  What Sampler.sample(cond=) and
    SDXLUNet.cond_term take."""
    _check(torch.is_tensor(zl) and zl.is_cuda and zl.dtype == torch.float32 and zl.dim() == 4
           and zl.permute(0, 2, 3, 1).is_contiguous(),
           "inpaint_cond: zl should be a channels-last fp32 [B, L, h, w] GPU tensor")
    B, L, h, w = zl.shape
    _check(1 <= L <= 7, "inpaint_cond: zl should have 1 to 7 channels")
    _check(torch.is_tensor(mask_lat) and mask_lat.device == zl.device and mask_lat.dtype == torch.float32
           and tuple(mask_lat.shape) in ((B, h, w), (B, 1, h, w)) and mask_lat.is_contiguous(),
           f"inpaint_cond: mask_lat should be a dense fp32 tensor of shape {(B, h, w)} or {(B, 1, h, w)} on zl's device")
    out = torch.empty((B, h, w, 8), dtype=torch.float16, device=zl.device)
    with torch.cuda.device(zl.device):
        code = _lib.mixdq_inpaint_cond_f16(mask_lat.data_ptr(), zl.data_ptr(), out.data_ptr(), B * h * w, L, _stream())
    _status(code, "inpaint_cond")
    return out.permute(0, 3, 1, 2)


def ip2p_cond(moments, rows=3, scale=1.0):
    """The conditioning channels of an 8-channel InstructPix2Pix UNet (mixdq_ip2p_cond_f16): moments fp16 [B, 2L, h, w] in
    channels-last storage (what VAEEncoder.moments returns), 1 <= L <= 8 -> fp16 [rows * B, 8, h, w] in channels-last
    storage, rows 1 or 3.  Row blocks in sampler_step3's order -- text + image, image only, neither: the first
    min(rows, 2) blocks hold f16(f32(mean) * scale) in channels 0..L-1 and +0.0 behind them, the third block is all +0.0.
    scale 1.0 returns the mean's own bits (latent_dist.mode(), unscaled: diffusers' InstructPix2Pix pipelines).  What
    Sampler.sample(cond=) and SDXLUNet.cond_term take."""
    _check(torch.is_tensor(moments) and moments.is_cuda and moments.dtype == torch.float16 and moments.dim() == 4
           and moments.shape[1] % 2 == 0 and moments.permute(0, 2, 3, 1).is_contiguous(),
           "ip2p_cond: moments should be a channels-last fp16 [B, 2L, h, w] GPU tensor")
    B, C2, h, w = moments.shape
    L = C2 // 2
    _check(1 <= L <= 8, "ip2p_cond: moments should hold 1 to 8 latent channels")
    _check(rows in (1, 3), "ip2p_cond: rows should be 1 or 3 (a two-row run cannot say which block is unconditioned)")
    out = torch.empty((rows * B, h, w, 8), dtype=torch.float16, device=moments.device)
    with torch.cuda.device(moments.device):
        code = _lib.mixdq_ip2p_cond_f16(moments.data_ptr(), out.data_ptr(), B, h * w, L, int(rows), float(scale),
                                        _stream())
    _status(code, "ip2p_cond")
    return out.permute(0, 3, 1, 2)


def composite_u8(decoded, original, mask):
    """The decoded image pasted into the original under the mask, as pixels (mixdq_composite_u8): decoded fp16
    [B, 3, H, W] (any strides: what VAEDecoder.decode returns), original uint8 [B, 3, H, W] (any strides), mask
    [B, H, W] or [B, 1, H, W] at image resolution (uint8 / fp16 / fp32, set as in mask_to_latent) -> uint8
    [B, 3, H, W] in channels-last storage: to_uint8(decoded) where the mask is set, the original's bytes elsewhere."""
    _check(torch.is_tensor(decoded) and decoded.is_cuda and decoded.dtype == torch.float16 and decoded.dim() == 4
           and decoded.shape[1] == 3, "composite_u8: decoded should be an fp16 [B, 3, H, W] GPU tensor")
    _check(torch.is_tensor(original) and original.device == decoded.device and original.dtype == torch.uint8
           and tuple(original.shape) == tuple(decoded.shape),
           "composite_u8: original should be a uint8 tensor of decoded's shape on its device")
    B, _, H, W = decoded.shape
    mB, mH, mW, mst = _mask3(mask, "composite_u8")
    _check(mask.device == decoded.device and (mB, mH, mW) == (B, H, W),
           "composite_u8: mask should have decoded's batch, height and width and be on its device")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=decoded.device)
    with torch.cuda.device(decoded.device):
        code = _lib.mixdq_composite_u8(decoded.data_ptr(), *decoded.stride(), original.data_ptr(), *original.stride(),
                                       mask.data_ptr(), IMAGE_DTYPES[mask.dtype], *mst, out.data_ptr(), B, H, W,
                                       _stream())
    _status(code, "composite_u8")
    return out.permute(0, 3, 1, 2)


_lib.mixdq_resample.argtypes = ([_vp, _i32] + [_i64] * 4 + [_i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32]
                                + [_i32] * 7 + [_vp])
_lib.mixdq_resample.restype = _i32
_lib.mixdq_resample_paste_u8.argtypes = ([_vp] + [_i64] * 4 + [_i32, _i32, _vp, _vp, _i32] + [_i64] * 3
                                         + [_i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32] + [_i32] * 6 + [_vp])
_lib.mixdq_resample_paste_u8.restype = _i32
_lib.mixdq_mask_bbox.argtypes = [_vp, _i32, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _vp]
_lib.mixdq_mask_bbox.restype = _i32
RESAMPLE_DST = {"u8": (0, torch.uint8), "u8_unit": (1, torch.uint8), "f32": (2, torch.float32)}   # MIXDQ_RESAMPLE_DST_*
RESAMPLE_MAX_TAPS = 256                                                   # MIXDQ_RESAMPLE_MAX_TAPS


def _tables(xs, wx, ys, wy, B, Hd, Wd, dev, what):
    """The four device tables of a resampling launch as (Bt, Tx, Ty): xs int32 [Bt, Wd], wx fp32 [Bt, Wd, Tx], ys int32
    [Bt, Hd], wy fp32 [Bt, Hd, Ty], dense, Bt 1 or B."""
    for tab, dt, nd in ((xs, torch.int32, 2), (wx, torch.float32, 3), (ys, torch.int32, 2), (wy, torch.float32, 3)):
        _check(torch.is_tensor(tab) and tab.device == dev and tab.dtype == dt and tab.dim() == nd
               and tab.is_contiguous(), f"{what}: tables should be dense int32 [Bt, n] / fp32 [Bt, n, T] tensors on "
               "the source's device")
    Bt = xs.shape[0]
    _check(Bt in (1, B) and wx.shape[0] == Bt and ys.shape[0] == Bt and wy.shape[0] == Bt,
           f"{what}: tables should have one leading entry, or one per image")
    _check(xs.shape[1] == Wd and wx.shape[1] == Wd and ys.shape[1] == Hd and wy.shape[1] == Hd,
           f"{what}: tables should have one row per output column / row")
    return Bt, wx.shape[2], wy.shape[2]


def resample(src, xs, wx, ys, wy, out="u8", mask=False):
    """The separable filter (mixdq_resample): src [B, C <= 4, Hs, Ws] uint8 / fp16 / fp32 of ANY strides, tables as
    mixdq_amd.image.resample_table / gaussian_table make them (xs int32 [Bt, Wd], wx fp32 [Bt, Wd, Tx], ys int32
    [Bt, Hd], wy fp32 [Bt, Hd, Ty]; Bt 1 or B) -> [B, C, Hd, Wd] in channels-last storage: 'u8' (mixdq_round_u8),
    'u8_unit' (mixdq_to_uint8: a source in [-1, 1]) or 'f32' (the accumulator).  mask=True: an element enters as 255
    where it is set (mask_to_latent's rule) and 0 elsewhere.  Arithmetic: include/mixdq_math.h mixdq_resample_tap."""
    _check(torch.is_tensor(src) and src.is_cuda and src.dim() == 4 and src.dtype in IMAGE_DTYPES,
           "resample: src should be a 4-D uint8, fp16 or fp32 GPU tensor")
    _check(out in RESAMPLE_DST, f"resample: out should be one of {tuple(RESAMPLE_DST)}")
    B, C, Hs, Ws = src.shape
    _check(1 <= C <= 4, "resample: src should have 1 to 4 channels")
    _check(torch.is_tensor(xs) and torch.is_tensor(ys) and xs.dim() == 2 and ys.dim() == 2, "resample: xs / ys should "
           "be 2-D tensors")
    Hd, Wd = ys.shape[1], xs.shape[1]
    Bt, Tx, Ty = _tables(xs, wx, ys, wy, B, Hd, Wd, src.device, "resample")
    kind, dt = RESAMPLE_DST[out]
    dst = torch.empty((B, Hd, Wd, C), dtype=dt, device=src.device)
    sb, sc, sh, sw = src.stride()
    with torch.cuda.device(src.device):
        code = _lib.mixdq_resample(src.data_ptr(), IMAGE_DTYPES[src.dtype], sb, sc, sh, sw, 1 if mask else 0,
                                   dst.data_ptr(), kind, xs.data_ptr(), wx.data_ptr(), Tx, ys.data_ptr(), wy.data_ptr(),
                                   Ty, Bt, B, C, Hs, Ws, Hd, Wd, _stream())
    _status(code, "resample")
    return dst.permute(0, 3, 1, 2)


def resample_paste_u8(decoded, out, mask, win, xs, wx, ys, wy, soft=False):
    """The crop workflow's way back, one launch, IN PLACE (mixdq_resample_paste_u8): decoded fp16 [B, 3, Hm, Wm] (any
    strides) is resized into window win[b] = (x0, y0, x1, y1) (int32 [B, 4] on the device) of `out`, uint8
    [B, 3, H, W] in channels-last storage holding the original, as mixdq_blend_u8(m, to_uint8(resized), out); mask
    [B, H, W] or [B, 1, H, W] of any strides: soft=True its uint8 bytes are m, otherwise m = 255 where it is set.
    Tables (window-relative, [Bt, Wt] / [Bt, Ht] with Wt, Ht the largest window) as in resample.  Returns `out`."""
    _check(torch.is_tensor(decoded) and decoded.is_cuda and decoded.dtype == torch.float16 and decoded.dim() == 4
           and decoded.shape[1] == 3, "resample_paste_u8: decoded should be an fp16 [B, 3, Hm, Wm] GPU tensor")
    B, _, Hm, Wm = decoded.shape
    _check(torch.is_tensor(out) and out.device == decoded.device and out.dtype == torch.uint8 and out.dim() == 4
           and out.shape[0] == B and out.shape[1] == 3 and out.permute(0, 2, 3, 1).is_contiguous(),
           "resample_paste_u8: out should be a uint8 [B, 3, H, W] tensor in channels-last storage on decoded's device")
    H, W = out.shape[2], out.shape[3]
    mB, mH, mW, mst = _mask3(mask, "resample_paste_u8")
    _check(mask.device == decoded.device and (mB, mH, mW) == (B, H, W),
           "resample_paste_u8: mask should have out's batch, height and width and be on its device")
    _check(not soft or mask.dtype == torch.uint8, "resample_paste_u8: a soft mask should be uint8")
    _check(torch.is_tensor(win) and win.device == decoded.device and win.dtype == torch.int32
           and tuple(win.shape) == (B, 4) and win.is_contiguous(), "resample_paste_u8: win should be an int32 [B, 4] "
           "tensor on decoded's device")
    _check(torch.is_tensor(xs) and torch.is_tensor(ys) and xs.dim() == 2 and ys.dim() == 2, "resample_paste_u8: xs / ys "
           "should be 2-D tensors")
    Ht, Wt = ys.shape[1], xs.shape[1]
    Bt, Tx, Ty = _tables(xs, wx, ys, wy, B, Ht, Wt, decoded.device, "resample_paste_u8")
    with torch.cuda.device(decoded.device):
        code = _lib.mixdq_resample_paste_u8(decoded.data_ptr(), *decoded.stride(), Hm, Wm, out.data_ptr(),
                                            mask.data_ptr(), IMAGE_DTYPES[mask.dtype], *mst, 1 if soft else 0,
                                            win.data_ptr(), xs.data_ptr(), wx.data_ptr(), Tx, ys.data_ptr(),
                                            wy.data_ptr(), Ty, Bt, Ht, Wt, B, H, W, _stream())
    _status(code, "resample_paste_u8")
    return out


def mask_bbox(mask):
    """The bounding boxes of a mask's set pixels (mixdq_mask_bbox): mask [B, H, W] or [B, 1, H, W], uint8 / fp16 / fp32
    of any strides -> int32 [B, 4] = (x0, y0, x1, y1) on the device, half-open, (0, 0, 0, 0) where nothing is set."""
    B, H, W, (sb, sh, sw) = _mask3(mask, "mask_bbox")
    out = torch.zeros((B, 4), dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        code = _lib.mixdq_mask_bbox(mask.data_ptr(), IMAGE_DTYPES[mask.dtype], sb, sh, sw, out.data_ptr(), B, H, W,
                                    _stream())
    _status(code, "mask_bbox")
    return out


_lib.mixdq_mask_dilate_u8.argtypes = [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp]
_lib.mixdq_mask_dilate_u8.restype = _i32
MASK_DILATE_MAX_RADIUS = 255


def mask_dilate(mask, radius):
    """A mask grown by `radius` pixels (mixdq_mask_dilate_u8): mask [B, H, W] or [B, 1, H, W], uint8 / fp16 / fp32 of
    any strides -> dense uint8 of the same shape, 255 where any set pixel (mask_to_latent's rule) lies within `radius`
    rows and columns -- a square window, PIL's ImageFilter.MaxFilter(2 * radius + 1) of the binarised mask -- and 0
    elsewhere; windows are clipped at the image border and never reach another image of the batch.  0 <= radius <=
    255; 0 binarises; a radius larger than the image is legal."""
    B, H, W, (sb, sh, sw) = _mask3(mask, "mask_dilate")
    _check(isinstance(radius, int) and not isinstance(radius, bool) and 0 <= radius <= MASK_DILATE_MAX_RADIUS,
           "mask_dilate: radius should be an int in [0, 255]")
    out = torch.empty(tuple(mask.shape), dtype=torch.uint8, device=mask.device)
    scratch = torch.empty((B, H, W), dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        code = _lib.mixdq_mask_dilate_u8(mask.data_ptr(), IMAGE_DTYPES[mask.dtype], sb, sh, sw, scratch.data_ptr(),
                                         out.data_ptr(), B, H, W, radius, _stream())
    _status(code, "mask_dilate")
    return out
