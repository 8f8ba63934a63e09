"""ctypes binding of the C ABI in include/psalm_hip.h (libpsalm_hip.so, hand-written gfx950 kernels).

PyTorch is used only as the device-memory container and stream owner: every method takes torch
tensors, checks layout, and hands raw `data_ptr()`s + sizes + the current HIP stream to the library.
There is NO fallback: if the library is missing, or a tensor is not on the GPU, this raises.

(The CPU test-suite constructs `Ops` over tests/emu/_build/libpsalm_emu.so -- the same kernel
sources compiled for the host -- explicitly via `Ops(path)`; `get_ops()` never does.)
"""
from __future__ import annotations

import ctypes
import math
import os
import sys
from ctypes import c_char_p, c_float, c_int, c_long, c_void_p
from typing import Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libpsalm_hip.so")

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_NEW = 0, 1, 2, 3
ACT_POST_RESIDUAL = 16
ACT_BIAS_ROW = 32
_DT = {torch.float32: F32, torch.bfloat16: BF16}


_DEBUG_SYNC = os.environ.get("PSALM_DEBUG_SYNC", "0") not in ("", "0")
# PSALM_DEBUG_BOUNDS=1: after every split-output GEMM, compare the magnitude BOUND behind its row scales with what the rows actually hold
# (one device round trip per call -- a debugging aid, off in production): the emitted operand keeps its 22 bits while bound / actual row
# maximum <= 2^14 (tests/test_2_gemm.py::test_gemm_x3_split_output_loose_bound); trained weights with outlier channels can be far looser
# than the seeded Gaussian ones of the tests, and this is how to find out.
_DEBUG_BOUNDS = os.environ.get("PSALM_DEBUG_BOUNDS", "0") not in ("", "0")
BOUND_LOOSENESS_LIMIT = 2.0 ** 14


class PsalmHipError(RuntimeError):
    pass


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise PsalmHipError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


ABI_VERSION = 19       # == PSALM_ABI_VERSION of include/psalm_hip.h (tests/test_0_abi.py compares the two and the built library's answer)


class _ProfiledLib:
    """Transparent proxy over the CDLL: when `records` is a list, every psalm_* launch is bracketed by a pair of
    HIP events on the launch stream (torch's current stream) so bench.py can attribute time per kernel family."""

    def __init__(self, cdll):
        object.__setattr__(self, "_cdll", cdll)
        object.__setattr__(self, "records", None)
        object.__setattr__(self, "calls", None)          # a list: the name of every psalm_* launch is appended (no events, no change of path)

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if not name.startswith("psalm_") or name in ("psalm_last_error", "psalm_backend", "psalm_abi_version", "psalm_gemm_last_kernel",
                                                         "psalm_gemm_set_tile_policy", "psalm_gemm_x3_set_products", "psalm_set_tuning",
                                                         "psalm_get_tuning") or name.endswith("_workspace"):
            return fn

        def call(*args):
            rec = self.records
            if self.calls is not None:
                self.calls.append(name)
            if _DEBUG_SYNC:
                # PSALM_DEBUG_SYNC=1: name every launch before it is issued and synchronise after it, so that a GPU memory
                # fault (which aborts the process asynchronously) is attributable: the last "launch" line without "ok".
                sys.stderr.write(f"[psalm launch] {name}\n"); sys.stderr.flush()
                rc = fn(*args)
                if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
                    torch.cuda.synchronize()
                sys.stderr.write(f"[psalm ok] {name}\n"); sys.stderr.flush()
                return rc
            if rec is None:
                return fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            kern = None
            if name.startswith(("psalm_gemm", "psalm_conv2d")):   # exact template instantiation the library launched (as a kernel trace names it)
                kern = self._cdll.psalm_gemm_last_kernel().decode()
            rec.append((name, tuple(a.value if hasattr(a, "value") else a for a in args), e0, e1, kern))
            return rc
        return call

    def __setattr__(self, k, v):
        if k in ("records", "calls"):
            object.__setattr__(self, k, v)
        else:
            setattr(self._cdll, k, v)


class SplitF16:
    """A matrix in split-f16 form (psalm_split_f16): `t` (rows, 2*Kp) float16 = [hi | lo], `inv_scale` (rows,) float32, logical
    shape (rows, K), Kp = ceil64(K).  Either operand of `Ops.gemm` may be one; in the "f16x3" mode GEMM weights are kept in this form."""
    __slots__ = ("t", "inv_scale", "K", "Kp")

    def __init__(self, t, inv_scale, K):
        self.t, self.inv_scale, self.K, self.Kp = t, inv_scale, K, t.shape[1] // 2

    @property
    def shape(self):
        return (self.t.shape[0], self.K)

    @property
    def dtype(self):
        return torch.float32                      # the values it stands for


class _PostDesc(ctypes.Structure):           # psalm_post_desc of include/psalm_hip.h
    _fields_ = [(n, c_int) for n in ("task", "Q", "h", "w", "Hpad", "Wpad", "crop_h", "crop_w", "out_h", "out_w", "C1", "n_region")] + \
               [("obj_thr", c_float), ("overlap_thr", c_float)]


class _PostIO(ctypes.Structure):             # psalm_post_io
    _fields_ = [(n, c_void_p) for n in ("pred_masks", "mask_up", "cls_logits", "seg_logits", "region_logits", "is_thing", "mask_pred", "sem_seg", "scores",
                                        "classes", "query", "inst_masks", "boxes", "pan", "counts")]


class _PhiLayer(ctypes.Structure):           # psalm_phi_layer of include/psalm_hip.h
    _fields_ = [("w1", c_void_p), ("w1_scale", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("w2_scale", c_void_p), ("b2", c_void_p),
                ("ln_g", c_void_p), ("ln_b", c_void_p), ("bnd", c_void_p), ("paired", c_int)]


class _RopeOut(ctypes.Structure):            # psalm_rope_out
    _fields_ = [("Qr", c_void_p), ("Kr", c_void_p), ("cos_table", c_void_p), ("sin_table", c_void_p), ("q_col", c_int), ("k_col", c_int),
                ("heads", c_int), ("B", c_int), ("L", c_int), ("Lp", c_int), ("scale", c_float), ("pad_", c_int)]


class _PhiDesc(ctypes.Structure):            # psalm_phi_desc
    _fields_ = [("num_layers", c_int), ("hidden", c_int), ("intermediate", c_int), ("heads", c_int), ("head_dim", c_int), ("rot", c_int),
                ("ln_eps", c_float), ("layers", ctypes.POINTER(_PhiLayer)), ("final_g", c_void_p), ("final_b", c_void_p)]


class _SwinBlock(ctypes.Structure):          # psalm_swin_block
    _fields_ = [(n, c_void_p) for n in ("n1_g", "n1_b", "n2_g", "n2_b", "qkv_w", "qkv_ws", "qkv_b", "qkv_bnd", "proj_w", "proj_ws", "proj_b",
                                         "fc1_w", "fc1_ws", "fc1_b", "fc1_bnd")] + [("fc1_paired", c_int)] + \
               [(n, c_void_p) for n in ("fc2_w", "fc2_ws", "fc2_b", "rpb")]


class _SwinStage(ctypes.Structure):          # psalm_swin_stage
    _fields_ = [("depth", c_int), ("heads", c_int), ("dim", c_int), ("blocks", ctypes.POINTER(_SwinBlock)), ("out_g", c_void_p), ("out_b", c_void_p),
                ("ds_g", c_void_p), ("ds_b", c_void_p), ("ds_w", c_void_p), ("ds_ws", c_void_p)]


class _SwinDesc(ctypes.Structure):           # psalm_swin_desc
    _fields_ = [("num_stages", c_int), ("patch", c_int), ("window", c_int), ("pe_kpad", c_int), ("mlp_ratio", c_int), ("pe_w", c_void_p),
                ("pe_ws", c_void_p), ("pe_b", c_void_p), ("pe_ln_g", c_void_p), ("pe_ln_b", c_void_p), ("stages", ctypes.POINTER(_SwinStage))]


class _ProjDesc(ctypes.Structure):           # psalm_projector_desc
    _fields_ = [("in_dim", c_int), ("mid_dim", c_int), ("out_dim", c_int)] + \
               [(n, c_void_p) for n in ("c1_w", "c1_ws", "c1_b", "c2_w", "c2_ws", "c2f_w", "c2f_ws", "c2f_b", "ds_w", "ds_ws", "ds_b", "fc_w", "fc_ws", "fc_b")]


class _PdEncLayer(ctypes.Structure):         # psalm_pd_enc_layer
    _fields_ = [(n, c_void_p) for n in ("value_w", "value_ws", "value_b", "ow_w", "ow_ws", "ow_b", "out_w", "out_ws", "out_b", "n1_g", "n1_b",
                                         "l1_w", "l1_ws", "l1_b", "l1_bnd")] + [("l1_paired", c_int)] + \
               [(n, c_void_p) for n in ("l2_w", "l2_ws", "l2_b", "n2_g", "n2_b")]


class _PdDesc(ctypes.Structure):             # psalm_pd_desc
    _fields_ = [("D", c_int), ("G", c_int), ("M", c_int), ("num_layers", c_int), ("ffn", c_int), ("mask_dim", c_int), ("in_dims", c_int * 4),
                ("ip_w", c_void_p * 3), ("ip_ws", c_void_p * 3), ("ip_b", c_void_p * 3), ("ip_gn_g", c_void_p * 3), ("ip_gn_b", c_void_p * 3)] + \
               [(n, c_void_p) for n in ("adapter_w", "adapter_ws", "adapter_b", "adapter_gn_g", "adapter_gn_b", "layer_w", "layer_ws", "layer_b",
                                         "layer_gn_g", "layer_gn_b", "mf_w", "mf_ws", "mf_b")] + [("layers", ctypes.POINTER(_PdEncLayer))]


class _PrLayer(ctypes.Structure):            # psalm_pr_layer
    _fields_ = [(n, c_void_p) for n in ("cq_w", "cq_b", "co_w", "co_b", "cn_g", "cn_b", "sqk_w", "sqk_b", "sv_w", "sv_b", "so_w", "so_b", "sn_g", "sn_b",
                                         "f1_w", "f1_b", "f2_w", "f2_b", "fn_g", "fn_b")]


class _PrDesc(ctypes.Structure):             # psalm_pr_desc
    _fields_ = [(n, c_int) for n in ("D", "heads", "Q", "num_layers", "num_levels", "ffn", "mask_dim")] + \
               [(n, c_void_p * 3) for n in ("lvl_k_w", "lvl_k_ws", "lvl_k_b", "lvl_v_w", "lvl_v_ws", "lvl_v_b")] + \
               [(n, c_void_p) for n in ("level_embed", "query_embed", "dn_g", "dn_b")] + [("mask_embed_w", c_void_p * 3), ("mask_embed_b", c_void_p * 3)] + \
               [(n, c_void_p * 2) for n in ("SEG_w", "SEG_b", "CLASS_w", "CLASS_b", "REGION_w", "REGION_b")] + [("layers", ctypes.POINTER(_PrLayer))]


class Ops:
    # psalm_gemm_set_tile_policy code of the library's default K loop for split-f16 GEMMs on 256 x 256 tiles (2580 K-panel form, 2581 32-deep
    # slices, 2582 slices with the all-padding m-tiles left out): what tests that switch it restore afterwards.
    GEMM_X3_256_DEFAULT = 2582

    def __init__(self, lib_path: str = DEFAULT_LIB):
        if not os.path.exists(lib_path):
            raise PsalmHipError(
                f"{lib_path} not found: build the HIP kernels first (python -m psalm_amd.build). "
                "psalm_amd has no CPU / PyTorch fallback by design.")
        cdll = ctypes.CDLL(lib_path)
        # the binary interface this binding was written against (include/psalm_hip.h PSALM_ABI_VERSION): checked BEFORE any other call -- a
        # stale prebuilt library would take this binding's integers for pointers (silent memory corruption, not an error)
        got = cdll.psalm_abi_version() if hasattr(cdll, "psalm_abi_version") else -1
        if got != ABI_VERSION:
            raise PsalmHipError(f"{lib_path}: psalm_abi_version() = {got}, this binding needs {ABI_VERSION}: rebuild the library "
                                "(python -m psalm_amd.build --force)")
        cdll.psalm_last_error.restype = c_char_p
        cdll.psalm_backend.restype = c_char_p
        cdll.psalm_gemm_last_kernel.restype = c_char_p
        self._cdll_raw = cdll
        self.lib = _ProfiledLib(cdll)
        self.backend = self.lib.psalm_backend().decode()
        self.is_emu = self.backend == "emu"
        self.device = torch.device("cpu") if self.is_emu else torch.device("cuda", torch.cuda.current_device())
        self.lib_path = lib_path
        self._ws = {}                      # cached kernel workspaces (device buffers owned by this binding)
        self._msda_tables = set()          # device-side MSDA level tables already validated (msda_forward_dev)
        self.debug_bounds = False          # True (or PSALM_DEBUG_BOUNDS=1): verify the scale bound of every split-output GEMM (host round trip)
        self.bound_looseness_max = 1.0
        self.x3 = False                    # True: float32 x float32 GEMMs run in split-f16 arithmetic (precision="f16x3")

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        if self.is_emu:
            return c_void_p(0)
        return c_void_p(torch.cuda.current_stream().cuda_stream)

    def _p(self, t: Optional[torch.Tensor]):
        if t is None:
            return c_void_p(0)
        if not t.is_contiguous():
            raise PsalmHipError("tensor must be contiguous")
        if self.is_emu:
            if t.device.type != "cpu":
                raise PsalmHipError("emulation backend needs CPU tensors")
        elif t.device.type != "cuda":
            raise PsalmHipError("psalm_amd kernels need GPU tensors (no CPU fallback)")
        return c_void_p(t.data_ptr())

    def _pv(self, t: Optional[torch.Tensor]):
        """pointer of a possibly row-strided view (caller passes the stride)."""
        if t is None:
            return c_void_p(0)
        if self.is_emu != (t.device.type == "cpu"):
            raise PsalmHipError("tensor on the wrong device for this backend (no CPU fallback)")
        return c_void_p(t.data_ptr())

    def _check(self, rc: int, name: str):
        if rc != 0:
            raise PsalmHipError(f"{name} failed (rc={rc}): {self.lib.psalm_last_error().decode()}")

    def _stage_ws(self, name, nbytes):
        """Workspace of a stage-level call: ONE buffer per (stage, launch stream), grown on demand and kept for the life of the binding (a
        fresh hundreds-of-MB torch.empty per call left the buffer's lifetime to the caching allocator's stream-ordered reuse and churned the allocator
        in eager mode).  A stage's successive calls on one stream are stream-ordered, so they may share it; calls on different streams get their own.
        While a hipGraph is being captured the buffer must belong to the capture's own pool: a fresh allocation then, as before."""
        if self.is_emu or torch.cuda.is_current_stream_capturing():
            return torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        key = ("stage_ws", name, torch.cuda.current_stream().cuda_stream)
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return t

    GEMM_WS_BYTES = 96 << 20

    def _gemm_ws(self):
        """Caller-owned split-K scratch handed to psalm_gemm: one buffer per launch stream for the life of the binding
        (two GEMMs on different streams may run concurrently and must not share partial-sum slabs)."""
        key = ("gemm", 0 if self.is_emu else torch.cuda.current_stream().cuda_stream)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(self.GEMM_WS_BYTES, dtype=torch.uint8, device=self.device)
        return ws

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        self._check(self.lib.psalm_memset_zero(self._p(t), c_long(t.numel() * t.element_size()), self._stream()), "psalm_memset_zero")
        return t

    def to_i64(self, t):
        """int32 vector -> int64 (psalm_cast_i32_i64): the reference's label / index tensors are LongTensors"""
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise PsalmHipError("to_i64: contiguous int32 tensor")
        out = self.empty(*t.shape, dtype=torch.int64)
        self._check(self.lib.psalm_cast_i32_i64(self._p(t), self._p(out), c_long(t.numel()), self._stream()), "psalm_cast_i32_i64")
        return out

    def copy_(self, dst, src):
        """dst <- src for two contiguous device tensors of equal dtype / numel, as a stream copy (no framework kernel)."""
        if dst.dtype != src.dtype or dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()) or src.device != dst.device:
            dst.copy_(src)
            return dst
        self._check(self.lib.psalm_copy_d2d(self._p(dst), self._p(src), c_long(dst.numel() * dst.element_size()), self._stream()), "psalm_copy_d2d")
        return dst

    # ------------------------------------------------------------------ GEMM
    def gemm(self, a, w, bias=None, residual=None, act=ACT_NONE, act_col_start=0, out=None, out_dtype=None):
        """out[M,N] = act(a[M,K] @ w[N,K]^T + bias) + residual.  `a`, `out`, `residual` may be row-strided 2-D views
        (last dim contiguous).  w.dtype selects the arithmetic: bfloat16 -> bf16 MFMA / fp32 accumulate,
        float32 -> exact fp32 MFMA."""
        if isinstance(a, SplitF16) or isinstance(w, SplitF16) or (self.x3 and a.dtype == torch.float32 and w.dtype == torch.float32):
            return self.gemm_x3(a, w, bias, residual, act, act_col_start, out, out_dtype)
        if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1]:
            raise PsalmHipError(f"gemm shape mismatch {tuple(a.shape)} x {tuple(w.shape)}")
        M, K = a.shape
        N = w.shape[0]
        if out is None:
            out = self.empty(M, N, dtype=out_dtype or (torch.float32 if w.dtype == torch.float32 else a.dtype))
        for t in (a, w, out) + ((residual,) if residual is not None else ()):
            if t.stride(-1) != 1:
                raise PsalmHipError("gemm operands need a contiguous last dimension")
        if residual is not None and (residual.dtype != out.dtype or residual.shape != out.shape):
            raise PsalmHipError("gemm residual must match the output's dtype and shape")
        if bias is not None and (bias.dtype != torch.float32 or bias.numel() != (M if act & ACT_BIAS_ROW else N)):
            raise PsalmHipError("gemm bias must be float32 (N,) -- or (M,) with ACT_BIAS_ROW")
        rc = self.lib.psalm_gemm(self._pv(a), _dt(a), c_long(a.stride(0)), self._pv(w), _dt(w), c_long(w.stride(0)),
                                 self._pv(bias), self._pv(residual), c_long(residual.stride(0) if residual is not None else 0),
                                 self._pv(out), _dt(out), c_long(out.stride(0)), M, N, K, act, act_col_start,
                                 self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_gemm")
        return out

    def split_f16(self, x):
        """x (rows,K) float32 (row-strided view) -> SplitF16: x * s = hi + lo in float16 with a per-row power-of-two scale."""
        if isinstance(x, SplitF16):
            return x
        if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
            raise PsalmHipError("split_f16: 2-D float32 input with a contiguous last dimension")
        rows, K = x.shape
        Kp = (K + 63) // 64 * 64
        t = self.empty(rows, 2 * Kp, dtype=torch.float16)
        inv = self.empty(rows, dtype=torch.float32)
        rc = self.lib.psalm_split_f16(self._pv(x), c_long(x.stride(0)), self._p(t), c_long(2 * Kp), self._p(inv), rows, K, self._stream())
        self._check(rc, "psalm_split_f16")
        return SplitF16(t, inv, K)

    def _x3_operands(self, a, w):
        """(a, w) for a split-f16 GEMM: float32 tensors are split on the fly."""
        a, w = self.split_f16(a), self.split_f16(w)
        if a.K != w.K or a.Kp != w.Kp:
            raise PsalmHipError(f"gemm shape mismatch {a.shape} x {w.shape}")
        return a, w

    def gemm_x3(self, a, w, bias=None, residual=None, act=ACT_NONE, act_col_start=0, out=None, out_dtype=None):
        """gemm() on split-f16 operands (float32 tensors are split on the fly): fp32-class result on the f16 matrix cores."""
        a, w = self._x3_operands(a, w)
        M, N = a.t.shape[0], w.t.shape[0]
        if out is None:
            if out_dtype not in (None, torch.float32):
                raise PsalmHipError("gemm_x3: float32 output only")
            out = self.empty(M, N, dtype=torch.float32)
        for t in (out,) + ((residual,) if residual is not None else ()):
            if t.dtype != torch.float32 or t.stride(-1) != 1 or tuple(t.shape) != (M, N):
                raise PsalmHipError("gemm_x3: float32 (M,N) output / residual with a contiguous last dimension")
        if bias is not None and (bias.dtype != torch.float32 or bias.numel() != (M if act & ACT_BIAS_ROW else N)):
            raise PsalmHipError("gemm bias must be float32 (N,) -- or (M,) with ACT_BIAS_ROW")
        rc = self.lib.psalm_gemm_x3(self._p(a.t), c_long(a.t.stride(0)), self._p(a.inv_scale), self._p(w.t), c_long(w.t.stride(0)),
                                    self._p(w.inv_scale), a.Kp, self._pv(bias), self._pv(residual),
                                    c_long(residual.stride(0) if residual is not None else 0), self._pv(out), c_long(out.stride(0)),
                                    M, N, act, act_col_start, self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_gemm_x3")
        return out

    def gemm_x3_ln_split(self, a, w, bias, residual, gamma, beta, eps, want_y=False):
        """x = a.w^T + bias + residual (float32), h = LayerNorm(x): returns (x, SplitF16(h), h float32 | None) -- the split-K reduce, the
        LayerNorm and the split of h are one row pass (psalm_gemm_x3_ln_split)."""
        a, w = self._x3_operands(a, w)
        M, N = a.t.shape[0], w.t.shape[0]
        if residual is not None and (residual.dtype != torch.float32 or tuple(residual.shape) != (M, N) or residual.stride(-1) != 1):
            raise PsalmHipError("gemm_x3_ln_split: float32 (M,N) residual")
        x = self.empty(M, N, dtype=torch.float32)
        y = self.empty(M, N, dtype=torch.float32) if want_y else None
        so, inv = self.empty(M, 2 * N, dtype=torch.float16), self.empty(M, dtype=torch.float32)
        rc = self.lib.psalm_gemm_x3_ln_split(self._p(a.t), c_long(a.t.stride(0)), self._p(a.inv_scale), self._p(w.t), c_long(w.t.stride(0)),
                                             self._p(w.inv_scale), a.Kp, self._pv(bias), self._pv(residual),
                                             c_long(residual.stride(0) if residual is not None else 0), self._p(x), c_long(N), M, N,
                                             self._p(gamma), self._p(beta), c_float(eps), self._pv(y), c_long(N), self._p(so), self._p(inv),
                                             self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_gemm_x3_ln_split")
        return x, SplitF16(so, inv, N), y

    def gemm_x3_split(self, a, w, bias, act, split_out, split_inv, bound_par, split_col_off=0, split_col_start=0, act_col_start=0,
                      out=None, global_rows=False, paired=False, rope=None):
        """gemm_x3 whose columns >= split_col_start are written as the split-f16 A operand of the next GEMM: into `split_out` (a SplitF16's
        .t buffer (M, 2*Kp_out) f16) at columns split_col_off.. (hi) / Kp_out + split_col_off.. (lo), row scales (inverse) into split_inv;
        bound_par: 4 device floats, see psalm_gemm_x3_split.  Columns below split_col_start go to `out` (M, >= split_col_start...) fp32.
        paired: the rows of `w` (and bias) >= split_col_start were permuted with `so_pair_perm` (stores straight from the accumulators).
        rope: dict(ws=, cos=, sin=, q_col=, k_col=, heads=, B=, L=) -- psalm_gemm_x3_split_rope: the k / q columns leave rotated (q scaled) in
        the attention workspace `ws` (causal_attention_workspace) instead of going to `out`."""
        a, w = self._x3_operands(a, w)
        M, N = a.t.shape[0], w.t.shape[0]
        if split_out.dtype != torch.float16 or split_out.dim() != 2 or split_out.shape[0] != M or split_out.stride(1) != 1:
            raise PsalmHipError("gemm_x3_split: split_out must be a (M, 2*Kp) float16 buffer")
        if split_inv.dtype != torch.float32 or split_inv.numel() != M or bound_par.dtype != torch.float32 or bound_par.numel() != 4:
            raise PsalmHipError("gemm_x3_split: split_inv (M,) / bound_par (4,) float32")
        if split_col_start > 0 and (out is None or out.dtype != torch.float32 or out.shape[0] != M or out.stride(-1) != 1):
            raise PsalmHipError("gemm_x3_split: float32 `out` required for the columns below split_col_start")
        if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N):
            raise PsalmHipError("gemm bias must be float32 (N,)")
        head = (self._p(a.t), c_long(a.t.stride(0)), self._p(a.inv_scale), self._p(w.t), c_long(w.t.stride(0)), self._p(w.inv_scale), a.Kp,
                self._pv(bias), self._pv(out), c_long(out.stride(0) if out is not None else 0), M, N, act, act_col_start, self._p(split_out),
                c_long(split_out.stride(0)), split_out.shape[1] // 2, split_col_off, split_col_start, int(bool(paired)), self._p(split_inv),
                self._p(bound_par), int(bool(global_rows)))
        tail = (self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        if rope is not None:
            B, L, heads = rope["B"], rope["L"], rope["heads"]
            Lp = (L + 31) // 32 * 32
            ws = rope["ws"]
            if ws.dtype != torch.uint8 or ws.numel() < self.causal_attention_workspace_bytes(B, L, heads) or ws.data_ptr() % 16:
                raise PsalmHipError("gemm_x3_split: rope['ws'] is a causal_attention_workspace(B, L, heads)")
            ro = _RopeOut(ws.data_ptr(), ws.data_ptr() + B * heads * Lp * 64 * 4, rope["cos"].data_ptr(), rope["sin"].data_ptr(), rope["q_col"],
                          rope["k_col"], heads, B, L, Lp, 1.0 / math.sqrt(64.0), 0)
            rc = self.lib.psalm_gemm_x3_split_rope(*head, ctypes.byref(ro), *tail)
            self._check(rc, "psalm_gemm_x3_split_rope")
        else:
            rc = self.lib.psalm_gemm_x3_split(*head, *tail)
            self._check(rc, "psalm_gemm_x3_split")
        if _DEBUG_BOUNDS or self.debug_bounds:
            self.check_split_bound(split_out, split_col_off, N - split_col_start, "gemm_x3_split")
        return split_out

    @staticmethod
    def so_pair_perm(n: int) -> torch.Tensor:
        """Row permutation of a weight (and its bias) whose GEMM emits split-f16 output with paired stores (psalm_gemm_x3_split,
        `paired`): index tensor `c` with W_physical = W_logical[c]; physical row 64 g + 32 b + j holds logical row 64 g + 2 j + b.  n % 64 == 0."""
        if n % 64:
            raise PsalmHipError("so_pair_perm: n % 64 == 0")
        p = torch.arange(n)
        return (p // 64) * 64 + 2 * (p % 32) + (p % 64) // 32

    def check_split_bound(self, split_out, col_off, ncols, what=""):
        """Looseness of the scale bound of an emitted split-f16 operand: the scale puts the BOUND in [2^12, 2^13), so 2^13 / max |hi| over a
        row's emitted columns is (within 2x) bound / actual row maximum.  Records the worst row in `bound_looseness_max`; raises beyond
        BOUND_LOOSENESS_LIMIT (lo would be reaching the f16 subnormal floor: the operand no longer carries 22 bits)."""
        hi = split_out[:, col_off:col_off + ncols].float().abs().amax(1)
        live = hi > 0
        if not bool(live.any()):
            return 1.0
        loose = float((2.0 ** 13 / hi[live]).max())
        self.bound_looseness_max = max(self.bound_looseness_max, loose)
        if loose > BOUND_LOOSENESS_LIMIT:
            raise PsalmHipError(f"{what}: the magnitude bound behind the split-f16 output scale is 2^{math.log2(loose):.1f} above the "
                                f"actual row maximum (limit 2^14): lo is reaching the f16 subnormal floor -- run this GEMM without the "
                                "fused split output (PSALM.fuse_split = False) or tighten its bound")
        return loose

    def gemm_ln(self, a, w, bias, residual, gamma, beta, eps=1e-5, ln_dtype=torch.bfloat16, act=ACT_NONE):
        """(C fp32, LayerNorm(C) ln_dtype) with C = act(a @ w^T + bias) + residual; bf16 a / w, K % 64 == 0."""
        M, K = a.shape
        N = w.shape[0]
        out = self.empty(M, N, dtype=torch.float32)
        ln_out = self.empty(M, N, dtype=ln_dtype)
        if residual is not None and (residual.dtype != torch.float32 or residual.shape != out.shape):
            raise PsalmHipError("gemm_ln: residual must be float32 (M,N)")
        rc = self.lib.psalm_gemm_ln(self._pv(a), _dt(a), c_long(a.stride(0)), self._pv(w), _dt(w), c_long(w.stride(0)), self._p(bias),
                                    self._pv(residual), c_long(residual.stride(0) if residual is not None else 0), self._p(out), F32,
                                    c_long(N), M, N, K, act, 0, self._p(gamma), self._p(beta), c_float(eps), self._p(ln_out), _dt(ln_out),
                                    c_long(N), self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_gemm_ln")
        return out, ln_out

    def conv2d_nhwc(self, x, B, H, W, wt, ksize, stride, pad, bias=None, residual=None, act=ACT_NONE, out_dtype=None):
        """Implicit-GEMM convolution: x (B*H*W, Cin) bf16 NHWC tokens, wt (Cout, k*k*Cin) bf16 (K order ky,kx,c) -> (B*Ho*Wo, Cout)."""
        Cin, Cout = x.shape[-1], wt.shape[0]
        if x.dtype != torch.bfloat16 or wt.dtype != torch.bfloat16 or wt.shape[1] != ksize * ksize * Cin:
            raise PsalmHipError("conv2d_nhwc: bf16 operands, weight (Cout, k*k*Cin)")
        Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        out = self.empty(B * Ho * Wo, Cout, dtype=out_dtype or x.dtype)
        if residual is not None and (residual.dtype != out.dtype or residual.shape != out.shape):
            raise PsalmHipError("conv2d_nhwc: residual must match the output")
        z = self._ws.get("zeros")
        if z is None:
            z = self._ws["zeros"] = torch.zeros(256, dtype=torch.uint8, device=self.device)
        rc = self.lib.psalm_conv2d_nhwc(self._p(x), B, H, W, Cin, self._p(wt), Cout, ksize, stride, pad, self._p(bias), self._pv(residual),
                                        c_long(residual.stride(0) if residual is not None else 0), self._p(out), _dt(out),
                                        c_long(out.stride(0)), act, self._p(z), self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES),
                                        self._stream())
        self._check(rc, "psalm_conv2d_nhwc")
        return out

    def gemm_describe(self, M, N, K, a_bf16=True, w_bf16=True, x3=False):
        """(path, BM, BN, splits) psalm_gemm / psalm_gemm_x3 (x3=True, K = 3*Kp) uses for this problem (path 1 = direct-to-LDS kernel)."""
        out = (c_int * 4)()
        if x3:
            self._cdll_raw.psalm_gemm_describe(M, N, K, 2, 2, c_long(self.GEMM_WS_BYTES), out)
            return tuple(out)
        self._cdll_raw.psalm_gemm_describe(M, N, K, BF16 if a_bf16 else F32, BF16 if w_bf16 else F32, c_long(self.GEMM_WS_BYTES), out)
        return tuple(out)

    def gemm_last_kernel(self) -> str:
        """template instantiation of this thread's last direct-to-LDS GEMM launch, as a kernel trace spells it"""
        return self._cdll_raw.psalm_gemm_last_kernel().decode()

    # ------------------------------------------------------------------ stage-level entries (csrc/stages.hip)
    def phi_desc(self, layers, hidden, intermediate, heads, head_dim, rot, ln_eps, final_g, final_b):
        """psalm_phi_desc for psalm_phi_forward.  layers: per Phi layer a dict(w1=SplitF16, b1=, w2=SplitF16, b2=, ln_g=, ln_b=, bnd=, paired=bool)
        of device tensors.  The returned object keeps the host array (and, through `keep`, the tensors) alive."""
        arr = (_PhiLayer * len(layers))()
        keep = []
        for i, ly in enumerate(layers):
            w1, w2 = ly["w1"], ly["w2"]
            if not (isinstance(w1, SplitF16) and isinstance(w2, SplitF16)):
                raise PsalmHipError("phi_desc: split-f16 weights (precision 'f16x3')")
            arr[i] = _PhiLayer(self._p(w1.t), self._p(w1.inv_scale), self._p(ly["b1"]), self._p(w2.t), self._p(w2.inv_scale), self._p(ly["b2"]),
                               self._p(ly["ln_g"]), self._p(ly["ln_b"]), self._p(ly["bnd"]), int(bool(ly["paired"])))
            keep.append(ly)
        d = _PhiDesc(len(layers), hidden, intermediate, heads, head_dim, rot, ln_eps, ctypes.cast(arr, ctypes.POINTER(_PhiLayer)),
                     self._p(final_g), self._p(final_b))
        d._keep = (arr, keep, final_g, final_b)
        return d

    def swin_desc(self, w, depths, heads, dims, patch, window, pe_kpad, mlp_ratio, paired):
        """psalm_swin_desc from the model's weight table `w` (names as PSALM._prepare_weights lays them out: swin{s}.{b}.qkv.w ...)."""
        keep, stages = [], (_SwinStage * len(depths))()

        def sp(name):                                # split-f16 weight -> (rows pointer, scales pointer)
            t = w[name]
            if not isinstance(t, SplitF16):
                raise PsalmHipError(f"swin_desc: {name} is not in split-f16 form (precision 'f16x3')")
            return self._p(t.t), self._p(t.inv_scale)
        for s_, (depth, nh, dim) in enumerate(zip(depths, heads, dims)):
            blocks = (_SwinBlock * depth)()
            for b in range(depth):
                q = f"swin{s_}.{b}."
                qw, qs = sp(q + "qkv.w"); pw_, ps_ = sp(q + "proj.w"); f1w, f1s = sp(q + "fc1.w"); f2w, f2s = sp(q + "fc2.w")
                blocks[b] = _SwinBlock(self._p(w[q + "n1.g"]), self._p(w[q + "n1.b"]), self._p(w[q + "n2.g"]), self._p(w[q + "n2.b"]), qw, qs,
                                       self._p(w[q + "qkv.b"]), self._p(w[q + "qkv.bnd"]), pw_, ps_, self._p(w[q + "proj.b"]), f1w, f1s,
                                       self._p(w[q + "fc1.b"]), self._p(w[q + "fc1.bnd"]), int(bool(paired.get(q + "fc1", False))), f2w, f2s,
                                       self._p(w[q + "fc2.b"]), self._p(w[q + "rpb"]))
            keep.append(blocks)
            last = s_ == len(depths) - 1
            dw, dsc = (c_void_p(0), c_void_p(0)) if last else sp(f"swin{s_}.ds.red.w")
            stages[s_] = _SwinStage(depth, nh, dim, ctypes.cast(blocks, ctypes.POINTER(_SwinBlock)), self._p(w[f"swin.out{s_}.g"]),
                                    self._p(w[f"swin.out{s_}.b"]), self._p(None if last else w[f"swin{s_}.ds.ln.g"]),
                                    self._p(None if last else w[f"swin{s_}.ds.ln.b"]), dw, dsc)
        pw0, ps0 = sp("swin.pe.w")
        d = _SwinDesc(len(depths), patch, window, pe_kpad, mlp_ratio, pw0, ps0, self._p(w["swin.pe.b"]), self._p(w["swin.pe.ln.g"]),
                      self._p(w["swin.pe.ln.b"]), ctypes.cast(stages, ctypes.POINTER(_SwinStage)))
        d._keep = (keep, stages, w)
        d._dims = list(dims)
        return d

    def swin_forward(self, desc, images):
        """SwinTransformer.forward as ONE native call (psalm_swin_forward): images (B,3,H,W) float32 -> [(tokens (B*h*w, C) float32, h, w)] per stage."""
        B, _, H, W = images.shape
        self.lib.psalm_swin_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_swin_forward_workspace(ctypes.byref(desc), B, H, W)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_swin_forward_workspace: {self.lib.psalm_last_error().decode()}")
        ws = self._stage_ws("swin", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        outs, hc, wc = [], (H + desc.patch - 1) // desc.patch, (W + desc.patch - 1) // desc.patch
        for C in desc._dims:
            outs.append((self.empty(B * hc * wc, C, dtype=torch.float32), hc, wc))
            hc, wc = (hc + 1) // 2, (wc + 1) // 2
        ptrs = (c_void_p * len(outs))(*[t.data_ptr() for t, _, _ in outs])
        rc = self.lib.psalm_swin_forward(ctypes.byref(desc), self._p(images), B, H, W, ptrs, c_void_p(ws.data_ptr() + off), c_long(nbytes),
                                         self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_swin_forward")
        return outs

    def projector_desc(self, w):
        def sp(name):
            t = w[name]
            if not isinstance(t, SplitF16):
                raise PsalmHipError(f"projector_desc: {name} is not in split-f16 form")
            return self._p(t.t), self._p(t.inv_scale)
        c1, c2, c2f, ds, fc = sp("proj.c1.w"), sp("proj.c2.w"), sp("proj.c2f.w"), sp("proj.ds.w"), sp("proj.fc.w")
        mid, cin = w["proj.c1.w"].t.shape[0], w["proj.ds.w"].K
        d = _ProjDesc(cin, mid, w["proj.fc.w"].t.shape[0], c1[0], c1[1], self._p(w["proj.c1.b"]), c2[0], c2[1], c2f[0], c2f[1], self._p(w["proj.c2f.b"]),
                      ds[0], ds[1], self._p(w["proj.ds.b"]), fc[0], fc[1], self._p(w["proj.fc.b"]))
        d._keep = w
        return d

    def projector_forward(self, desc, res5, B, h, w_):
        """The conv projector as ONE native call (psalm_projector_forward): res5 (B*h*w, C) float32 -> ((B*ho*wo, hidden) float32, ho*wo)."""
        self.lib.psalm_projector_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_projector_forward_workspace(ctypes.byref(desc), B, h, w_)
        if nbytes < 0:
            raise PsalmHipError("psalm_projector_forward_workspace: bad descriptor / geometry")
        ws = self._stage_ws("projector", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        ho, wo = (h + 2 - 3) // 2 + 1, (w_ + 2 - 3) // 2 + 1
        out = self.empty(B * ho * wo, desc.out_dim, dtype=torch.float32)
        rc = self.lib.psalm_projector_forward(ctypes.byref(desc), self._p(res5), B, h, w_, self._p(out), c_void_p(ws.data_ptr() + off), c_long(nbytes),
                                              self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_projector_forward")
        return out, ho * wo

    def pd_desc(self, w, D, G, M, num_layers, ffn, mask_dim, in_dims, paired):
        def sp(name):
            t = w[name]
            if not isinstance(t, SplitF16):
                raise PsalmHipError(f"pd_desc: {name} is not in split-f16 form")
            return t.t.data_ptr(), t.inv_scale.data_ptr()

        def P(name):
            return w[name].data_ptr()
        layers = (_PdEncLayer * num_layers)()
        for i in range(num_layers):
            q = f"pd.enc{i}."
            v, ow, ou, l1, l2 = sp(q + "value.w"), sp(q + "ow.w"), sp(q + "out.w"), sp(q + "l1.w"), sp(q + "l2.w")
            layers[i] = _PdEncLayer(v[0], v[1], P(q + "value.b"), ow[0], ow[1], P(q + "ow.b"), ou[0], ou[1], P(q + "out.b"), P(q + "n1.g"), P(q + "n1.b"),
                                    l1[0], l1[1], P(q + "l1.b"), P(q + "l1.bnd"), int(bool(paired.get(q + "l1", False))), l2[0], l2[1], P(q + "l2.b"),
                                    P(q + "n2.g"), P(q + "n2.b"))
        ips = [sp(f"pd.ip{i}.w") for i in range(3)]
        ad, la, mf = sp("pd.adapter.w"), sp("pd.layer.w"), sp("pd.mf.w")
        V3 = c_void_p * 3
        d = _PdDesc(D, G, M, num_layers, ffn, mask_dim, (c_int * 4)(*in_dims), V3(*[x[0] for x in ips]), V3(*[x[1] for x in ips]),
                    V3(*[P(f"pd.ip{i}.b") for i in range(3)]), V3(*[P(f"pd.ip{i}.gn.g") for i in range(3)]), V3(*[P(f"pd.ip{i}.gn.b") for i in range(3)]),
                    ad[0], ad[1], P("pd.adapter.b"), P("pd.adapter.gn.g"), P("pd.adapter.gn.b"), la[0], la[1], P("pd.layer.b"), P("pd.layer.gn.g"),
                    P("pd.layer.gn.b"), mf[0], mf[1], P("pd.mf.b"), ctypes.cast(layers, ctypes.POINTER(_PdEncLayer)))
        d._keep = (layers, w)
        return d

    def pixel_decoder_forward(self, desc, feats, lvl_pos):
        """MSDeformAttn pixel decoder of ONE image as ONE native call.  feats: [(tokens (h*w, C) float32 contiguous, h, w)] res2..res5.
        Returns (mask_features (h2*w2, mask_dim), ms (S, D) level-concatenated [res5 | res4 | res3])."""
        hw = (c_int * 8)(*[int(v) for _, h, w_ in feats for v in (h, w_)])
        self.lib.psalm_pixel_decoder_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_pixel_decoder_forward_workspace(ctypes.byref(desc), hw)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_pixel_decoder_forward_workspace: {self.lib.psalm_last_error().decode()}")
        ws = self._stage_ws("pixel_decoder", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        for t, _, _ in feats:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise PsalmHipError("pixel_decoder_forward: contiguous float32 feature tokens")
        S = sum(h * w_ for _, h, w_ in feats[1:])
        mf = self.empty(feats[0][1] * feats[0][2], desc.mask_dim, dtype=torch.float32)
        ms = self.empty(S, desc.D, dtype=torch.float32)
        ptrs = (c_void_p * 4)(*[t.data_ptr() for t, _, _ in feats])
        rc = self.lib.psalm_pixel_decoder_forward(ctypes.byref(desc), ptrs, hw, self._p(lvl_pos), self._p(mf), self._p(ms), c_void_p(ws.data_ptr() + off),
                                                  c_long(nbytes), self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_pixel_decoder_forward")
        return mf, ms

    def pr_desc(self, w, D, heads, Q, num_layers, num_levels, ffn, mask_dim):
        def P(name):
            t = w[name]
            if isinstance(t, SplitF16) or t.dtype != torch.float32:
                raise PsalmHipError(f"pr_desc: {name} must be a plain float32 tensor")
            return t.data_ptr()
        layers = (_PrLayer * num_layers)()
        for i in range(num_layers):
            q = f"pr{i}."
            layers[i] = _PrLayer(*[P(q + n) for n in ("cq.w", "cq.b", "co.w", "co.b", "cn.g", "cn.b", "sqk.w", "sqk.b", "sv.w", "sv.b", "so.w", "so.b", "sn.g",
                                                      "sn.b", "f1.w", "f1.b", "f2.w", "f2.b", "fn.g", "fn.b")])
        V3, V2 = c_void_p * 3, c_void_p * 2
        ks = [w[f"pr.lvl{l}.k.w"] for l in range(num_levels)] + [None] * (3 - num_levels)
        vs = [w[f"pr.lvl{l}.v.w"] for l in range(num_levels)] + [None] * (3 - num_levels)
        if not all(t is None or isinstance(t, SplitF16) for t in ks + vs):
            raise PsalmHipError("pr_desc: the level K / V projection weights must be in split-f16 form")
        pb = lambda t, f: 0 if t is None else f(t)               # noqa: E731
        d = _PrDesc(D, heads, Q, num_layers, num_levels, ffn, mask_dim,
                    V3(*[pb(t, lambda x: x.t.data_ptr()) for t in ks]), V3(*[pb(t, lambda x: x.inv_scale.data_ptr()) for t in ks]),
                    V3(*[P(f"pr.lvl{l}.k.b") if l < num_levels else 0 for l in range(3)]),
                    V3(*[pb(t, lambda x: x.t.data_ptr()) for t in vs]), V3(*[pb(t, lambda x: x.inv_scale.data_ptr()) for t in vs]),
                    V3(*[P(f"pr.lvl{l}.v.b") if l < num_levels else 0 for l in range(3)]),
                    P("pr.level_embed"), P("pr.query_embed"), P("pr.dn.g"), P("pr.dn.b"),
                    V3(*[P(f"pr.mask_embed{j}.w") for j in range(3)]), V3(*[P(f"pr.mask_embed{j}.b") for j in range(3)]),
                    V2(*[P(f"pr.SEG_proj{j}.w") for j in range(2)]), V2(*[P(f"pr.SEG_proj{j}.b") for j in range(2)]),
                    V2(*[P(f"pr.CLASS_proj{j}.w") for j in range(2)]), V2(*[P(f"pr.CLASS_proj{j}.b") for j in range(2)]),
                    V2(*[P(f"pr.REGION_proj{j}.w") for j in range(2)]), V2(*[P(f"pr.REGION_proj{j}.b") for j in range(2)]),
                    ctypes.cast(layers, ctypes.POINTER(_PrLayer)))
        d._keep = (layers, w)
        return d

    def predictor_kv(self, desc, ms, shapes, prpos, mf, mf_size, n_reg=0, slot=0, own=False):
        """The LLM-independent front of the masked-attention decoder (psalm_predictor_kv: level K / V projections + mask-feature split) into a workspace
        that `predictor_forward(..., kv=<the returned handle>)` then continues in.  `slot`: which of the caller's images this is (each keeps its own
        workspace until its predictor call).  own = True: a fresh buffer the returned handle owns instead of the binding's per-slot one (image sessions keep
        the front across calls: the forward call only reads it)."""
        H2, W2 = mf_size
        hw = (c_int * (2 * len(shapes)))(*[int(v) for s_ in shapes for v in s_])
        self.lib.psalm_predictor_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_predictor_forward_workspace(ctypes.byref(desc), hw, H2, W2, int(n_reg))
        if nbytes < 0:
            raise PsalmHipError(f"psalm_predictor_forward_workspace: {self.lib.psalm_last_error().decode()}")
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device) if own else self._stage_ws(f"predictor{slot}", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        VP = c_void_p * len(shapes)
        rc = self.lib.psalm_predictor_kv(ctypes.byref(desc), VP(*[t.data_ptr() for t in ms]), hw, VP(*[t.data_ptr() for t in prpos]), self._p(mf), H2, W2, int(n_reg),
                                         c_void_p(ws.data_ptr() + off), c_long(nbytes), self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_predictor_kv")
        return (ws, off, nbytes, int(n_reg))

    def predictor_forward(self, desc, ms, shapes, prpos, mf, mf_size, seg_query, class_emb=None, seg_emb=None, region_emb=None, kv=None):
        """The masked-attention decoder of ONE image as ONE native call.  ms / prpos: per-level (h*w, D) float32 tensors; mf (H2*W2, mask_dim);
        seg_query (Q, D); *_emb (n, D) float32 or None.  Returns (pred_masks (Q, H2*W2), cls_logits | None, seg_logits | None, region_logits | None)."""
        H2, W2 = mf_size
        Q, D = desc.Q, desc.D
        for t in list(ms) + list(prpos) + [mf, seg_query] + [e for e in (class_emb, seg_emb, region_emb) if e is not None]:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
                raise PsalmHipError("predictor_forward: contiguous, 16-byte aligned float32 tensors")
        hw = (c_int * (2 * len(shapes)))(*[int(v) for s_ in shapes for v in s_])
        n_reg = int(region_emb.shape[0]) if region_emb is not None else 0
        self.lib.psalm_predictor_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_predictor_forward_workspace(ctypes.byref(desc), hw, H2, W2, n_reg)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_predictor_forward_workspace: {self.lib.psalm_last_error().decode()}")
        if kv is not None:
            ws, off, kv_bytes, kv_reg = kv
            if kv_bytes != nbytes or kv_reg != n_reg:
                raise PsalmHipError("predictor_forward: the K / V workspace was prepared for another geometry / region count")
        else:
            ws = self._stage_ws("predictor", nbytes + 256)
            off = (-ws.data_ptr()) % 256
        masks = self.empty(Q, H2 * W2, dtype=torch.float32)
        cls = self.empty(Q, class_emb.shape[0], dtype=torch.float32) if class_emb is not None else None
        seg = self.empty(Q, seg_emb.shape[0], dtype=torch.float32) if seg_emb is not None else None
        reg = self.empty(n_reg, Q, dtype=torch.float32) if region_emb is not None else None
        VP = c_void_p * len(shapes)
        rc = self.lib.psalm_predictor_forward(ctypes.byref(desc), VP(*[t.data_ptr() for t in ms]), hw, VP(*[t.data_ptr() for t in prpos]), self._p(mf), H2, W2,
                                              self._p(seg_query), self._p(class_emb), int(class_emb.shape[0]) if class_emb is not None else 0, self._p(seg_emb),
                                              int(seg_emb.shape[0]) if seg_emb is not None else 0, self._p(region_emb), n_reg, self._p(masks), self._p(cls),
                                              self._p(seg), self._p(reg), c_void_p(ws.data_ptr() + off), c_long(nbytes), self._p(self._gemm_ws()),
                                              c_long(self.GEMM_WS_BYTES), 1 if kv is not None else 0, self._stream())
        self._check(rc, "psalm_predictor_forward")
        return masks, cls, seg, reg

    def predictor_kv_bytes(self, desc, shapes, mf_size):
        """bytes of the front psalm_predictor_kv writes (and psalm_predictor_forward_batched reads) at the start of its workspace"""
        hw = (c_int * (2 * len(shapes)))(*[int(v) for s_ in shapes for v in s_])
        self.lib.psalm_predictor_kv_bytes.restype = c_long
        n = self.lib.psalm_predictor_kv_bytes(ctypes.byref(desc), hw, int(mf_size[0]), int(mf_size[1]))
        if n < 0:
            raise PsalmHipError(f"psalm_predictor_kv_bytes: {self.lib.psalm_last_error().decode()}")
        return int(n)

    def predictor_forward_batched(self, desc, shapes, kv, mf, mf_size, seg_query, class_emb=None, cls_counts=None, seg_emb=None, seg_counts=None,
                                  region_emb=None, reg_counts=None, offsets=None):
        """The masked-attention decoder for B prompts of ONE image as ONE native call over B * Q query rows (psalm_predictor_forward_batched).
        kv: `predictor_kv`'s handle (only read; any region count); seg_query (B*Q, D); *_emb: the prompts' embeddings packed in prompt order, *_counts
        their per-prompt row counts (or offsets = {"cls" | "seg" | "region": (B + 1) offsets} given verbatim).  Returns (pred_masks (B*Q, H2*W2),
        cls_logits, seg_logits, region_logits): the logits packed -- prompt b's (Q, n_b) block (region: (n_b, Q)) behind those of the prompts before
        it, flat float32 -- or None.  The scratch is a per-stage workspace of the binding."""
        H2, W2 = mf_size
        Q, D = desc.Q, desc.D
        if seg_query.dim() != 2 or seg_query.shape[0] % Q:
            raise PsalmHipError("predictor_forward_batched: seg_query (B*Q, D)")
        B = int(seg_query.shape[0]) // Q
        for t in [mf, seg_query] + [e for e in (class_emb, seg_emb, region_emb) if e is not None]:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
                raise PsalmHipError("predictor_forward_batched: contiguous, 16-byte aligned float32 tensors")
        offsets = offsets or {}

        def offs(name, emb, counts):
            if emb is None:
                return None, 0
            o_ = offsets.get(name)
            if o_ is None:
                if counts is None or len(counts) != B:
                    raise PsalmHipError(f"predictor_forward_batched: one {name} count per prompt")
                o_ = [0]
                for c in counts:
                    o_.append(o_[-1] + int(c))
                if o_[-1] != emb.shape[0]:
                    raise PsalmHipError(f"predictor_forward_batched: the {name} counts do not add up to the embedding rows")
            o_ = [int(v) for v in o_]
            if len(o_) != B + 1 or o_[-1] > emb.shape[0]:
                raise PsalmHipError(f"predictor_forward_batched: (B + 1) {name} offsets within the embedding rows")
            return (c_int * (B + 1))(*o_), max(o_[-1], 0)

        c_off, n_c = offs("cls", class_emb, cls_counts)
        s_off, n_s = offs("seg", seg_emb, seg_counts)
        r_off, n_r = offs("region", region_emb, reg_counts)
        hw = (c_int * (2 * len(shapes)))(*[int(v) for s_ in shapes for v in s_])
        self.lib.psalm_predictor_forward_batched_workspace.restype = c_long
        nbytes = self.lib.psalm_predictor_forward_batched_workspace(ctypes.byref(desc), hw, H2, W2, B, n_r)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_predictor_forward_batched_workspace: {self.lib.psalm_last_error().decode()}")
        kws, koff, kbytes, _ = kv
        if kbytes < self.predictor_kv_bytes(desc, shapes, mf_size):
            raise PsalmHipError("predictor_forward_batched: the K / V workspace was prepared for another geometry")
        ws = self._stage_ws("predictor_batched", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        masks = self.empty(B * Q, H2 * W2, dtype=torch.float32)
        cls = self.empty(Q * n_c, dtype=torch.float32) if class_emb is not None else None
        seg = self.empty(Q * n_s, dtype=torch.float32) if seg_emb is not None else None
        reg = self.empty(n_r * Q, dtype=torch.float32) if region_emb is not None else None
        rc = self.lib.psalm_predictor_forward_batched(ctypes.byref(desc), hw, c_void_p(kws.data_ptr() + koff), self._p(mf), H2, W2, B, self._p(seg_query),
                                                      self._p(class_emb), c_off, self._p(seg_emb), s_off, self._p(region_emb), r_off, self._p(masks),
                                                      self._p(cls), self._p(seg), self._p(reg), c_void_p(ws.data_ptr() + off), c_long(nbytes),
                                                      self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_predictor_forward_batched")
        return masks, cls, seg, reg

    POST_TASKS = {"semantic": 0, "instance": 1, "panoptic": 2, "referring": 3, "region": 4}

    def postprocess(self, task, sizes, pred_masks=None, mask_up=None, cls_logits=None, seg_logits=None, region_logits=None, is_thing=None,
                    obj_thr=0.8, overlap_thr=0.8, counts_extra=0):
        """llava_phi.py:1401-1466 for one image as ONE native call (psalm_postprocess_<task>): sizes = (Hpad, Wpad, crop_h, crop_w, out_h, out_w);
        pred_masks (Q,h,w) and / or mask_up (Q,Hpad,Wpad) float32.  Returns a dict of the result tensors at their maximum sizes (the caller slices by
        `counts` after its one read-back): mask_pred, sem_seg, scores, classes, query, inst_masks, boxes, pan, counts -- those the task has.
        counts_extra: int32 words allocated behind the 2 + 3 Q the call writes (the caller's own small results, fetched with the same read-back)."""
        Hpad, Wpad, oh, ow, height, width = [int(v) for v in sizes]
        src = pred_masks if pred_masks is not None else mask_up
        Q = int(src.shape[0])
        h_, w_ = (int(pred_masks.shape[1]), int(pred_masks.shape[2])) if pred_masks is not None else (Hpad, Wpad)
        C1 = int(cls_logits.shape[1]) if cls_logits is not None else 0
        k = int(region_logits.shape[0]) if region_logits is not None else 0
        code = self.POST_TASKS[task]
        d = _PostDesc(code, Q, h_, w_, Hpad, Wpad, oh, ow, height, width, C1, k, float(obj_thr), float(overlap_thr))
        self.lib.psalm_postprocess_workspace.restype = c_long
        nbytes = self.lib.psalm_postprocess_workspace(ctypes.byref(d), 1 if mask_up is not None else 0)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_postprocess_workspace: {self.lib.psalm_last_error().decode()}")
        ws = self._stage_ws("postprocess", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        resize_after = (oh, ow, height, width) != (Hpad, Wpad, Hpad, Wpad)
        out = {}
        if task == "semantic":
            if mask_up is None:
                out["mask_pred"] = self.empty(Q, Hpad, Wpad)
            out["sem_seg"] = self.empty(C1 - 1, height, width)
        else:
            if resize_after or mask_up is None:
                out["mask_pred"] = self.empty(Q, height, width)
            out["scores"] = self.empty(Q, k) if task == "region" else self.empty(Q)
            out["inst_masks"] = self.empty(Q, height, width)
            out["boxes"] = self.empty(Q, 4)
            out["counts"] = self.empty(2 + 3 * Q + int(counts_extra), dtype=torch.int32)
            if task in ("instance", "panoptic"):
                out["classes"] = self.empty(Q, dtype=torch.int64)
            if task != "region":
                out["query"] = self.empty(Q, dtype=torch.int64)
            if task == "panoptic":
                out["sem_seg"] = self.empty(C1 - 1, height, width)
                out["pan"] = self.empty(height, width, dtype=torch.int32)
        io = _PostIO(*[self._pi(t) for t in (pred_masks, mask_up, cls_logits, seg_logits, region_logits, is_thing, out.get("mask_pred"), out.get("sem_seg"),
                                             out.get("scores"), out.get("classes"), out.get("query"), out.get("inst_masks"), out.get("boxes"), out.get("pan"),
                                             out.get("counts"))])
        which = c_int(0)
        fn = getattr(self.lib, "psalm_postprocess_" + task)
        rc = fn(ctypes.byref(d), ctypes.byref(io), ctypes.byref(which), c_void_p(ws.data_ptr() + off), c_long(nbytes), self._stream())
        self._check(rc, "psalm_postprocess_" + task)
        if which.value == 1:
            out["mask_pred"] = mask_up
        return out

    @staticmethod
    def _pi(t):
        return None if t is None else t.data_ptr()

    def phi_forward_plan(self, desc, B, L):
        """psalm_phi_forward_plan: (q / k rotated in the GEMM epilogue, launches per layer, launches in front of the layer loop) of phi_forward"""
        out = (c_int * 3)()
        self._check(self._cdll_raw.psalm_phi_forward_plan(ctypes.byref(desc), B, L, out), "psalm_phi_forward_plan")
        return bool(out[0]), out[1], out[2]

    def phi_forward(self, desc, embeds, key_mask, cos, sin, B, L):
        """PhiModel.forward over inputs_embeds (B*L, hidden) float32 as ONE native call (psalm_phi_forward): returns the final-LayerNorm hidden
        states (B*L, hidden) float32.  Same bits as PSALM.llm's op-by-op sequence, which keeps the RoPE pre-pass per layer; the native call
        rotates q / k in the [k|v|q|fc1] GEMM's epilogue where `phi_forward_plan` says so (TUNE_PHI_ROPE_EPILOGUE)."""
        if embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[0] != B * L or embeds.shape[1] != desc.hidden:
            raise PsalmHipError("phi_forward: float32 (B*L, hidden) embeddings")
        self.lib.psalm_phi_forward_workspace.restype = c_long
        nbytes = self.lib.psalm_phi_forward_workspace(ctypes.byref(desc), B, L)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_phi_forward_workspace: {self.lib.psalm_last_error().decode()}")
        ws = self._stage_ws("phi", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        out = self.empty(B * L, desc.hidden, dtype=torch.float32)
        rc = self.lib.psalm_phi_forward(ctypes.byref(desc), self._p(embeds), self._p(key_mask), self._p(cos), self._p(sin), B, L, self._p(out),
                                        c_void_p(ws.data_ptr() + off), c_long(nbytes), self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES),
                                        self._stream())
        self._check(rc, "psalm_phi_forward")
        return out

    # ---- image sessions: the Phi pass cut behind the prompt-independent prefix (psalm_phi_prefix / psalm_phi_suffix)
    def phi_prefix_cache(self, hidden, heads, P, num_layers):
        """A fresh prefix cache + its per-layer (K (heads, ceil32 P, 64), V (P, hidden)) float32 views; the layout is the library's
        (psalm_phi_prefix_cache_layer_bytes: what psalm_phi_prefix writes and psalm_phi_suffix reads)."""
        self.lib.psalm_phi_prefix_cache_layer_bytes.restype = c_long
        kb, vb = c_long(0), c_long(0)
        stride = self.lib.psalm_phi_prefix_cache_layer_bytes(hidden, heads, P, ctypes.byref(kb), ctypes.byref(vb))
        if stride <= 0:
            raise PsalmHipError("phi_prefix_cache: hidden, heads, P >= 1")
        kb, Pp = kb.value, (P + 31) // 32 * 32
        raw = torch.empty(stride * num_layers + 256, dtype=torch.uint8, device=self.device)
        off = (-raw.data_ptr()) % 256
        buf = raw[off:off + stride * num_layers]
        views = []
        for i in range(num_layers):
            o0 = stride * i
            views.append((buf[o0:o0 + heads * Pp * 64 * 4].view(torch.float32).view(heads, Pp, 64),
                          buf[o0 + kb:o0 + kb + P * hidden * 4].view(torch.float32).view(P, hidden)))
        return buf, views

    def phi_prefix(self, desc, embeds, key_mask, cos, sin, P, cache):
        """psalm_phi_prefix: the Phi layers over the P prefix rows as ONE native call; fills `cache` (phi_prefix_cache's buffer)."""
        if embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[0] != P or embeds.shape[1] != desc.hidden or key_mask.numel() != P:
            raise PsalmHipError("phi_prefix: float32 (P, hidden) embeddings, key mask of P bytes")
        self.lib.psalm_phi_prefix_workspace.restype = c_long
        self.lib.psalm_phi_prefix_cache_bytes.restype = c_long
        nbytes = self.lib.psalm_phi_prefix_workspace(ctypes.byref(desc), P)
        cbytes = self.lib.psalm_phi_prefix_cache_bytes(ctypes.byref(desc), P)
        if nbytes < 0 or cbytes < 0:
            raise PsalmHipError(f"psalm_phi_prefix_workspace: {self.lib.psalm_last_error().decode()}")
        if cache.numel() < cbytes or cache.data_ptr() % 256:
            raise PsalmHipError("phi_prefix: cache of psalm_phi_prefix_cache_bytes() bytes, 256-byte aligned")
        ws = self._stage_ws("phi_prefix", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        rc = self.lib.psalm_phi_prefix(ctypes.byref(desc), self._p(embeds), self._p(key_mask), self._p(cos), self._p(sin), P, self._p(cache),
                                       c_long(cache.numel()), c_void_p(ws.data_ptr() + off), c_long(nbytes), self._p(self._gemm_ws()),
                                       c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_phi_prefix")

    def phi_suffix(self, desc, embeds, key_mask, cos, sin, N, S, P, cache):
        """psalm_phi_suffix: the Phi layers over the N*S suffix rows against the prefix cache as ONE native call: final-LayerNorm hidden states
        (N*S, hidden) float32.  Same launches, same order, same bits as PSALM._llm_session's op-by-op sequence."""
        if embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[0] != N * S or embeds.shape[1] != desc.hidden or key_mask.numel() != N * S \
                or cos.shape[0] < P + S:
            raise PsalmHipError("phi_suffix: float32 (N*S, hidden) embeddings, key mask (N, S), tables of >= P + S rows")
        self.lib.psalm_phi_suffix_workspace.restype = c_long
        self.lib.psalm_phi_prefix_cache_bytes.restype = c_long
        nbytes = self.lib.psalm_phi_suffix_workspace(ctypes.byref(desc), N, S)
        cbytes = self.lib.psalm_phi_prefix_cache_bytes(ctypes.byref(desc), P)
        if nbytes < 0 or cbytes < 0:
            raise PsalmHipError(f"psalm_phi_suffix_workspace: {self.lib.psalm_last_error().decode()}")
        if cache.numel() < cbytes or cache.data_ptr() % 256:
            raise PsalmHipError("phi_suffix: cache of psalm_phi_prefix_cache_bytes() bytes, 256-byte aligned")
        ws = self._stage_ws("phi_suffix", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        out = self.empty(N * S, desc.hidden, dtype=torch.float32)
        rc = self.lib.psalm_phi_suffix(ctypes.byref(desc), self._p(embeds), self._p(key_mask), self._p(cos), self._p(sin), N, S, P, self._p(cache),
                                       c_long(cache.numel()), self._p(out), c_void_p(ws.data_ptr() + off), c_long(nbytes),
                                       self._p(self._gemm_ws()), c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_phi_suffix")
        return out

    def phi_suffix_grouped(self, desc, embeds, key_mask, cos, sin, N, S, refs, P_max, table=None):
        """psalm_phi_suffix_grouped: phi_suffix for prompts of several sessions -- `refs`: the (num_layers, N) table of prefix_ref_table, as a host
        array (uploaded here) or already on the device as bytes (then `table`, its host copy, is what gets checked)."""
        if embeds.dtype != torch.float32 or embeds.dim() != 2 or embeds.shape[0] != N * S or embeds.shape[1] != desc.hidden or key_mask.numel() != N * S \
                or cos.shape[0] < P_max + S:
            raise PsalmHipError("phi_suffix_grouped: float32 (N*S, hidden) embeddings, key mask (N, S), tables of >= P_max + S rows")
        refs = self._prefix_refs(refs, table, desc.num_layers * N, P_max, desc.heads, "phi_suffix_grouped")
        self.lib.psalm_phi_suffix_grouped_workspace.restype = c_long
        nbytes = self.lib.psalm_phi_suffix_grouped_workspace(ctypes.byref(desc), N, S)
        if nbytes < 0:
            raise PsalmHipError(f"psalm_phi_suffix_grouped_workspace: {self.lib.psalm_last_error().decode()}")
        ws = self._stage_ws("phi_suffix", nbytes + 256)
        off = (-ws.data_ptr()) % 256
        out = self.empty(N * S, desc.hidden, dtype=torch.float32)
        rc = self.lib.psalm_phi_suffix_grouped(ctypes.byref(desc), self._p(embeds), self._p(key_mask), self._p(cos), self._p(sin), N, S,
                                               self._p(refs) if refs is not None else None, P_max, self._p(out),
                                               c_void_p(ws.data_ptr() + off), c_long(nbytes), self._p(self._gemm_ws()),
                                               c_long(self.GEMM_WS_BYTES), self._stream())
        self._check(rc, "psalm_phi_suffix_grouped")
        return out

    def x3_products(self, n: int):
        """f16 products formed per algorithmic product by this thread's split-f16 GEMMs: 3 (default, fp32-class) or 1 (hi.hi only: plain f16
        operands, a third of the matrix work -- the reduced-precision LLM side mode, not at the parity bar).  See psalm_gemm_x3_set_products."""
        self._check(self.lib.psalm_gemm_x3_set_products(int(n)), "psalm_gemm_x3_set_products")

    TUNE_GEMM_XCD_KSPLIT, TUNE_ATTN_XCD_HEADS, TUNE_GEMM_MID, TUNE_DECODER_FUSE, TUNE_ROW_GROUPS, TUNE_MHA_QTILE_WAVES = 0, 1, 2, 3, 4, 5      # PSALM_TUNE_* of include/psalm_hip.h
    TUNE_PHI_ROPE_EPILOGUE = 6

    def set_tuning(self, key: int, value: int):
        """psalm_set_tuning: process-wide atomic switches between kernel forms with identical results (A/B runs, tests)."""
        self._check(self.lib.psalm_set_tuning(int(key), int(value)), "psalm_set_tuning")

    def get_tuning(self, key: int) -> int:
        return int(self.lib.psalm_get_tuning(int(key)))

    def gemm_tile_policy(self, bm: int):
        """0 = automatic, 256 / 128 / 64 = force the direct-to-LDS kernel's tile height (tuning / tests)."""
        self._check(self.lib.psalm_gemm_set_tile_policy(bm), "psalm_gemm_set_tile_policy")

    # ------------------------------------------------------------------ row ops
    def layernorm(self, x, gamma, beta, eps=1e-5, out=None, out_dtype=None, out2=None, add=None, out3=None):
        """LayerNorm over the last dim of a 2-D (row-strided) view.  out2: optional bf16 (rows,C) second copy;
        out3: optional bf16 (rows,C) = result + add[row % add.shape[0]] (add fp32 (r,C))."""
        rows, C = x.shape
        if out is None:
            out = self.empty(rows, C, dtype=out_dtype or x.dtype)
        for t in (out2, out3):
            if t is not None and t.dtype != torch.bfloat16:
                raise PsalmHipError("layernorm: out2 / out3 must be bfloat16")
        if out3 is not None and (add is None or add.dtype != torch.float32 or add.shape[1] != C):
            raise PsalmHipError("layernorm: out3 needs a float32 (r,C) `add` table")
        rc = self.lib.psalm_layernorm3(self._pv(x), _dt(x), c_long(x.stride(0)), self._pv(out), _dt(out), c_long(out.stride(0)),
                                       self._pv(out2), c_long(out2.stride(0) if out2 is not None else 0),
                                       self._p(add) if out3 is not None else c_void_p(0), c_long(add.shape[0] if out3 is not None else 0),
                                       self._pv(out3), c_long(out3.stride(0) if out3 is not None else 0),
                                       self._p(gamma), self._p(beta), rows, C, c_float(eps), self._stream())
        self._check(rc, "psalm_layernorm3")
        return out

    def layernorm_split(self, x, gamma, beta, eps=1e-5, want_y=False, want_split=True, add=None):
        """LayerNorm of float32 rows whose result leaves as the next GEMM's split-f16 A operand (f16x3 mode).
        Returns (y float32 | None, SplitF16(y) | None, SplitF16(y + add[row % r]) | None)."""
        rows, C = x.shape
        if x.dtype != torch.float32 or x.stride(1) != 1:
            raise PsalmHipError("layernorm_split: float32 rows")
        Kp = (C + 63) // 64 * 64
        y = self.empty(rows, C, dtype=torch.float32) if want_y else None
        s1 = i1 = s2 = i2 = None
        if want_split:
            s1, i1 = self.empty(rows, 2 * Kp, dtype=torch.float16), self.empty(rows, dtype=torch.float32)
        if add is not None:
            if add.dtype != torch.float32 or add.shape[1] != C:
                raise PsalmHipError("layernorm_split: float32 (r,C) `add` table")
            s2, i2 = self.empty(rows, 2 * Kp, dtype=torch.float16), self.empty(rows, dtype=torch.float32)
        rc = self.lib.psalm_layernorm_split(self._pv(x), c_long(x.stride(0)), self._p(y), c_long(C), self._p(gamma), self._p(beta), rows, C,
                                            c_float(eps), self._p(s1), self._p(i1), self._p(add), c_long(add.shape[0] if add is not None else 0),
                                            self._p(s2), self._p(i2), self._stream())
        self._check(rc, "psalm_layernorm_split")
        return y, (SplitF16(s1, i1, C) if want_split else None), (SplitF16(s2, i2, C) if add is not None else None)

    def swin_window_gather(self, x, gamma, beta, B, H, W, ws, shift, eps=1e-5, out_dtype=None):
        """x (B*H*W, C) -> LN + pad + roll(-shift) + window partition -> (B*nW*ws*ws, C)."""
        C = x.shape[-1]
        nWh, nWw = (H + ws - 1) // ws, (W + ws - 1) // ws
        out = self.empty(B * nWh * nWw * ws * ws, C, dtype=out_dtype or x.dtype)
        rc = self.lib.psalm_swin_window_gather(self._p(x), _dt(x), self._p(out), _dt(out), self._p(gamma), self._p(beta), B, H, W,
                                               C, ws, shift, c_float(eps), self._stream())
        self._check(rc, "psalm_swin_window_gather")
        return out

    def swin_window_gather_split(self, x, gamma, beta, B, H, W, ws, shift, eps=1e-5):
        """swin_window_gather whose rows leave as the qkv GEMM's split-f16 A operand (f16x3 mode): x (B*H*W, C) float32 -> SplitF16."""
        C = x.shape[-1]
        if x.dtype != torch.float32 or C % 8 or C > 2048:
            raise PsalmHipError("swin_window_gather_split: float32, C % 8 == 0, C <= 2048")
        nWh, nWw = (H + ws - 1) // ws, (W + ws - 1) // ws
        rows, Kp = B * nWh * nWw * ws * ws, (C + 63) // 64 * 64
        t = self.empty(rows, 2 * Kp, dtype=torch.float16)
        inv = self.empty(rows, dtype=torch.float32)
        rc = self.lib.psalm_swin_window_gather_split(self._p(x), self._p(t), self._p(inv), self._p(gamma), self._p(beta), B, H, W, C, ws, shift,
                                                     c_float(eps), self._stream())
        self._check(rc, "psalm_swin_window_gather_split")
        return SplitF16(t, inv, C)

    def swin_window_merge_ln_split(self, win, shortcut, gamma, beta, B, H, W, ws, shift, eps=1e-5):
        """swin_window_merge_ln with norm2's result as the fc1 GEMM's split-f16 A operand: (x_new float32, SplitF16(LayerNorm(x_new)))."""
        C = shortcut.shape[-1]
        if shortcut.dtype != torch.float32 or win.dtype != torch.float32 or C % 8 or C > 2048:
            raise PsalmHipError("swin_window_merge_ln_split: float32 operands, C % 8 == 0, C <= 2048")
        rows, Kp = shortcut.shape[0], (C + 63) // 64 * 64
        out_x = torch.empty_like(shortcut)
        t = self.empty(rows, 2 * Kp, dtype=torch.float16)
        inv = self.empty(rows, dtype=torch.float32)
        rc = self.lib.psalm_swin_window_merge_ln_split(self._p(win), self._p(shortcut), self._p(out_x), self._p(t), self._p(inv), self._p(gamma),
                                                       self._p(beta), B, H, W, C, ws, shift, c_float(eps), self._stream())
        self._check(rc, "psalm_swin_window_merge_ln_split")
        return out_x, SplitF16(t, inv, C)

    def swin_window_merge(self, win, shortcut, B, H, W, ws, shift, out=None):
        """out (B*H*W, C) = shortcut + window_reverse/roll(+shift)/crop(win)."""
        C = shortcut.shape[-1]
        if out is None:
            out = torch.empty_like(shortcut)
        rc = self.lib.psalm_swin_window_merge(self._p(win), _dt(win), self._p(shortcut), self._p(out), _dt(shortcut), B, H, W, C,
                                              ws, shift, self._stream())
        self._check(rc, "psalm_swin_window_merge")
        return out

    def swin_window_merge_ln(self, win, shortcut, gamma, beta, B, H, W, ws, shift, eps=1e-5, h_dtype=None):
        """(x_new fp32, LayerNorm(x_new) h_dtype): window_reverse/roll/crop + residual fused with the block's norm2."""
        C = shortcut.shape[-1]
        if shortcut.dtype != torch.float32:
            raise PsalmHipError("swin_window_merge_ln: the residual stream must be float32")
        out_x = torch.empty_like(shortcut)
        out_h = self.empty(shortcut.shape[0], C, dtype=h_dtype or win.dtype)
        rc = self.lib.psalm_swin_window_merge_ln(self._p(win), _dt(win), self._p(shortcut), self._p(out_x), self._p(out_h), _dt(out_h),
                                                 self._p(gamma), self._p(beta), B, H, W, C, ws, shift, c_float(eps), self._stream())
        self._check(rc, "psalm_swin_window_merge_ln")
        return out_x, out_h

    def patch_merge_ln(self, x, gamma, beta, B, H, W, eps=1e-5, out_dtype=None):
        C = x.shape[-1]
        out = self.empty(B * ((H + 1) // 2) * ((W + 1) // 2), 4 * C, dtype=out_dtype or x.dtype)
        rc = self.lib.psalm_patch_merge_ln(self._p(x), _dt(x), self._p(out), _dt(out), self._p(gamma), self._p(beta), B, H, W, C,
                                           c_float(eps), self._stream())
        self._check(rc, "psalm_patch_merge_ln")
        return out

    def groupnorm_nhwc(self, x, gamma, beta, B, HW, groups, eps=1e-5, relu=False, out_dtype=None, out=None):
        """x (B*HW, C) NHWC -> GroupNorm(groups) [+ReLU]."""
        C = x.shape[-1]
        if out is None:
            out = self.empty(B * HW, C, dtype=out_dtype or x.dtype)
        ws = self.empty(B * ((HW + 63) // 64 + 1) * groups * 2, dtype=torch.float32)
        rc = self.lib.psalm_groupnorm_nhwc(self._p(x), _dt(x), self._p(out), _dt(out), self._p(gamma), self._p(beta), self._p(ws),
                                           B, HW, C, groups, c_float(eps), int(relu), self._stream())
        self._check(rc, "psalm_groupnorm_nhwc")
        return out

    def layernorm_chain(self, x, g1, b1, add=None, g2=None, b2=None, eps=1e-5):
        """(y1, y2 | None, y3 | None) = (LN(x; g1, b1), y1 + add[row % add_rows], LN(y1; g2, b2)) in one launch (psalm_layernorm_chain, fp32)."""
        rows, C = x.shape
        y1 = self.empty(rows, C, dtype=torch.float32)
        y2 = self.empty(rows, C, dtype=torch.float32) if add is not None else None
        y3 = self.empty(rows, C, dtype=torch.float32) if g2 is not None else None
        rc = self.lib.psalm_layernorm_chain(self._p(x), c_long(x.stride(0)), self._p(y1), c_long(C), self._p(g1), self._p(b1), self._pv(add),
                                            c_long(add.shape[0] if add is not None else 0), self._pv(y2), c_long(C), self._pv(g2), self._pv(b2),
                                            self._pv(y3), c_long(C), rows, C, c_float(eps), self._stream())
        self._check(rc, "psalm_layernorm_chain")
        return y1, y2, y3

    def gemm_f32_pair(self, a0, w0, bias0, a1, w1, bias1, act0=ACT_NONE, act1=ACT_NONE):
        """two exact-fp32 skinny GEMMs in one launch (psalm_gemm_f32_pair): returns (a0 . w0^T + bias0, a1 . w1^T + bias1)"""
        c0 = self.empty(a0.shape[0], w0.shape[0], dtype=torch.float32)
        c1 = self.empty(a1.shape[0], w1.shape[0], dtype=torch.float32)
        rc = self.lib.psalm_gemm_f32_pair(self._p(a0), self._p(w0), self._pv(bias0), self._p(c0), a0.shape[0], w0.shape[0], a0.shape[1], act0,
                                          self._p(a1), self._p(w1), self._pv(bias1), self._p(c1), a1.shape[0], w1.shape[0], a1.shape[1], act1, self._stream())
        self._check(rc, "psalm_gemm_f32_pair")
        return c0, c1

    def gemm_f32_rows(self, a, w, bias=None, residual=None, act=ACT_NONE):
        """act(a . w^T + bias) + residual on the exact-fp32 skinny kernel over cdiv(M, 32) row tiles (psalm_gemm_f32_rows; M <= 2048, N <= 8192):
        row r carries the words gemm() returns for any <= 192-row set holding it.  a / residual may be row-strided float32 views."""
        M, K = a.shape
        N = w.shape[0]
        out = self.empty(M, N, dtype=torch.float32)
        rc = self.lib.psalm_gemm_f32_rows(self._pv(a), c_long(a.stride(0)), self._pv(w), c_long(w.stride(0)), self._pv(bias), self._pv(residual),
                                          c_long(residual.stride(0) if residual is not None else 0), self._p(out), c_long(N), M, N, K, act, self._stream())
        self._check(rc, "psalm_gemm_f32_rows")
        return out

    def gemm_f32_rows_pair(self, a0, w0, bias0, a1, w1, bias1, act0=ACT_NONE, act1=ACT_NONE):
        """gemm_f32_pair with M <= 2048 (psalm_gemm_f32_rows_pair)"""
        c0 = self.empty(a0.shape[0], w0.shape[0], dtype=torch.float32)
        c1 = self.empty(a1.shape[0], w1.shape[0], dtype=torch.float32)
        rc = self.lib.psalm_gemm_f32_rows_pair(self._p(a0), self._p(w0), self._pv(bias0), self._p(c0), a0.shape[0], w0.shape[0], a0.shape[1], act0,
                                               self._p(a1), self._p(w1), self._pv(bias1), self._p(c1), a1.shape[0], w1.shape[0], a1.shape[1], act1, self._stream())
        self._check(rc, "psalm_gemm_f32_rows_pair")
        return c0, c1

    def gemm_f32_grouped(self, a_list, w_list):
        """[a_i . w_i^T] for <= 16 (a_i (M_i, K), w_i (N_i, K)) contiguous float32 pairs of one K in ONE launch (psalm_gemm_f32_grouped; M_i <= 192)"""
        n = len(a_list)
        if n != len(w_list) or not 1 <= n <= 16:
            raise PsalmHipError("gemm_f32_grouped: 1..16 problems")
        K = int(a_list[0].shape[1])
        for a, w in zip(a_list, w_list):
            if a.dtype != torch.float32 or w.dtype != torch.float32 or a.dim() != 2 or w.dim() != 2 or a.shape[1] != K or w.shape[1] != K:
                raise PsalmHipError("gemm_f32_grouped: float32 (M_i, K) x (N_i, K) operands of one K")
        outs = [self.empty(a.shape[0], w.shape[0], dtype=torch.float32) for a, w in zip(a_list, w_list)]
        VP, VI = c_void_p * n, c_int * n
        rc = self.lib.psalm_gemm_f32_grouped(VP(*[self._p(a).value or 0 for a in a_list]), VP(*[self._p(w).value or 0 for w in w_list]),
                                             VP(*[self._p(c).value or 0 for c in outs]), VI(*[int(a.shape[0]) for a in a_list]),
                                             VI(*[int(w.shape[0]) for w in w_list]), K, n, self._stream())
        self._check(rc, "psalm_gemm_f32_grouped")
        return outs

    def add_bcast(self, a, b, out_dtype=None):
        """out[r] = a[r] + b[r % b_rows]   (a (rows,C), b (b_rows,C))."""
        rows, C = a.shape
        out = self.empty(rows, C, dtype=out_dtype or a.dtype)
        rc = self.lib.psalm_add_bcast(self._p(a), _dt(a), self._p(b), _dt(b), self._p(out), _dt(out), c_long(rows), C,
                                      c_long(b.shape[0]), self._stream())
        self._check(rc, "psalm_add_bcast")
        return out

    def gather_rows(self, srcs, src_id, src_row, C, out_dtype=torch.float32):
        """dst[r] = srcs[src_id[r]][src_row[r]]; src_id < 0 -> zero row.  src_id/src_row int32 device tensors."""
        srcs = list(srcs) + [None] * (4 - len(srcs))
        rows = src_id.numel()
        out = self.empty(rows, C, dtype=out_dtype)
        args = []
        for t in srcs:
            args += [self._p(t), _dt(t) if t is not None else 0]
        rc = self.lib.psalm_gather_rows(*args, self._p(src_id), self._p(src_row), self._p(out), _dt(out), c_long(rows), C,
                                        self._stream())
        self._check(rc, "psalm_gather_rows")
        return out

    def segment_mean(self, x, seg_offsets, seg_rows, out_dtype=None):
        """out[s] = mean of x[seg_rows[seg_offsets[s]:seg_offsets[s+1]]]."""
        nseg = seg_offsets.numel() - 1
        C = x.shape[-1]
        out = self.empty(nseg, C, dtype=out_dtype or x.dtype)
        rc = self.lib.psalm_segment_mean(self._pv(x), _dt(x), c_long(x.stride(0)), self._p(seg_offsets), self._p(seg_rows),
                                         self._p(out), _dt(out), nseg, C, self._stream())
        self._check(rc, "psalm_segment_mean")
        return out

    # ------------------------------------------------------------------ attention
    def window_attention(self, qkv, bias_table, B, nWh, nWw, heads, ws, shift):
        C = qkv.shape[-1] // 3
        out = self.empty(qkv.shape[0], C, dtype=qkv.dtype)
        if qkv.dtype == torch.bfloat16 and ws == 12:          # matrix-core kernel (bf16 mode)
            rc = self.lib.psalm_window_attention_mfma(self._p(qkv), self._p(bias_table), self._p(out), B, nWh, nWw, C, heads, ws,
                                                      shift, self._stream())
            self._check(rc, "psalm_window_attention_mfma")
            return out
        rc = self.lib.psalm_window_attention(self._p(qkv), self._p(bias_table), self._p(out), _dt(qkv), B, nWh, nWw, C, heads, ws,
                                             shift, self._stream())
        self._check(rc, "psalm_window_attention")
        return out

    def window_attention_split(self, qkv, bias_table, a_inv, bound_par, B, nWh, nWw, heads, ws, shift):
        """window_attention on a float32 qkv buffer (12 x 12 windows) -> SplitF16 (rows, C): the projection GEMM's A operand, see
        psalm_window_attention_split.  a_inv: row scales of the qkv GEMM's A operand; bound_par: >= 2 device floats."""
        C = qkv.shape[-1] // 3
        if qkv.dtype != torch.float32 or ws != 12 or a_inv.numel() != qkv.shape[0]:
            raise PsalmHipError("window_attention_split: float32 qkv, 12 x 12 windows, one operand scale per row")
        Kp = (C + 63) // 64 * 64
        so = (self.empty if Kp == C else self.zeros)(qkv.shape[0], 2 * Kp, dtype=torch.float16)
        inv = self.empty(qkv.shape[0], dtype=torch.float32)
        rc = self.lib.psalm_window_attention_split(self._p(qkv), self._p(bias_table), self._p(a_inv), self._p(bound_par), self._p(so), Kp,
                                                   self._p(inv), B, nWh, nWw, C, heads, ws, shift, self._stream())
        self._check(rc, "psalm_window_attention_split")
        return SplitF16(so, inv, C)

    def causal_attention(self, buf, q_off, k_off, v_off, out, o_off, cos, sin, key_mask, B, L, heads, head_dim, rot):
        """buf (B*L, ld) holds q|k|v column blocks; out (B*L, ldo) receives the attention output at column o_off.
        bf16 buffers run on the matrix cores (psalm_causal_attention_mfma); fp32 buffers on the exact fp32 kernel."""
        if buf.dtype != out.dtype:
            raise PsalmHipError("causal_attention: buf/out dtype mismatch")
        if buf.dtype == torch.bfloat16:
            self.lib.psalm_causal_attention_mfma_workspace.restype = c_long
            nbytes = self.lib.psalm_causal_attention_mfma_workspace(B, L, heads)
            key = ("causal_ws", nbytes)
            ws = self._ws.get(key)
            if ws is None:
                ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            rc = self.lib.psalm_causal_attention_mfma(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._pv(out),
                                                      c_long(out.stride(0)), o_off, self._p(cos), self._p(sin), self._p(key_mask),
                                                      self._p(ws), B, L, heads, head_dim, rot, self._stream())
            self._check(rc, "psalm_causal_attention_mfma")
            return out
        if (buf.dtype == torch.float32 and head_dim == 64 and rot == 32 and buf.stride(0) % 4 == 0 and out.stride(0) % 4 == 0
                and all(v % 4 == 0 for v in (q_off, k_off, v_off, o_off)) and buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0):
            self.lib.psalm_causal_attention_f32_workspace.restype = c_long      # fp32 matrix-core kernel, key-split inside the block
            nbytes = self.lib.psalm_causal_attention_f32_workspace(B, L, heads)
            key = ("causal_f32_ws", nbytes)
            ws = self._ws.get(key)
            if ws is None:
                ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            rc = self.lib.psalm_causal_attention_f32(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._pv(out),
                                                     c_long(out.stride(0)), o_off, self._p(cos), self._p(sin), self._p(key_mask), self._p(ws),
                                                     B, L, heads, head_dim, rot, self._stream())
            self._check(rc, "psalm_causal_attention_f32")
            return out
        rc = self.lib.psalm_causal_attention(self._pv(buf), _dt(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._pv(out),
                                             c_long(out.stride(0)), o_off, self._p(cos), self._p(sin), self._p(key_mask), B, L,
                                             heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_causal_attention")
        return out

    def causal_attention_workspace_bytes(self, B, L, heads):
        self.lib.psalm_causal_attention_f32_workspace.restype = c_long
        return self.lib.psalm_causal_attention_f32_workspace(B, L, heads)

    def causal_attention_workspace(self, B, L, heads):
        """The fp32 Phi attention's workspace, [Qr | Kr | Mk | Tk] (psalm_causal_attention_f32_workspace bytes): the one `causal_attention` and
        `causal_attention_split` use for this shape, for the two-step form (phi_attention_tables, gemm_x3_split(rope=), causal_attention_split_prepared)."""
        nbytes = self.causal_attention_workspace_bytes(B, L, heads)
        key = ("causal_f32_ws", nbytes)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def phi_attention_tables(self, key_mask, ws, B, L, heads):
        """psalm_phi_attention_tables: Mk / Tk of `ws` from key_mask (B, L) u8, zeros in the padding rows of Qr / Kr -- once per forward pass."""
        if key_mask.dtype != torch.uint8 or key_mask.numel() != B * L or not key_mask.is_contiguous():
            raise PsalmHipError("phi_attention_tables: contiguous uint8 key mask (B, L)")
        if ws.dtype != torch.uint8 or ws.numel() < self.causal_attention_workspace_bytes(B, L, heads):
            raise PsalmHipError("phi_attention_tables: workspace of causal_attention_workspace(B, L, heads)")
        self._check(self.lib.psalm_phi_attention_tables(self._p(key_mask), self._p(ws), B, L, heads, self._stream()), "psalm_phi_attention_tables")

    def causal_attention_split_prepared(self, buf, v_off, split_out, split_inv, split_col_off, ws, B, L, heads, head_dim):
        """causal_attention_split's attention kernel alone, on a workspace whose Qr / Kr / Mk / Tk are in place (phi_attention_tables +
        gemm_x3_split(rope=)); `buf` holds the v columns at v_off."""
        if buf.dtype != torch.float32 or split_out.dtype != torch.float16 or split_inv.dtype != torch.float32:
            raise PsalmHipError("causal_attention_split_prepared: float32 v buffer, float16 split buffer, float32 scales")
        if ws.dtype != torch.uint8 or ws.numel() < self.causal_attention_workspace_bytes(B, L, heads):
            raise PsalmHipError("causal_attention_split_prepared: workspace of causal_attention_workspace(B, L, heads)")
        rc = self.lib.psalm_causal_attention_f32_split_prepared(self._pv(buf), c_long(buf.stride(0)), v_off, self._p(split_out),
                                                                c_long(split_out.stride(0)), split_out.shape[1] // 2, split_col_off,
                                                                self._p(split_inv), self._p(ws), B, L, heads, head_dim, self._stream())
        self._check(rc, "psalm_causal_attention_f32_split_prepared")
        return split_out

    def causal_attention_split(self, buf, q_off, k_off, v_off, split_out, split_inv, split_col_off, cos, sin, key_mask, B, L, heads,
                               head_dim, rot):
        """causal_attention on an fp32 buffer whose output goes, in split-f16 form under the row scales 1/split_inv, into columns
        split_col_off.. of `split_out` ((B*L, 2*Kp) float16; lo part Kp columns further) -- see psalm_causal_attention_f32_split."""
        if buf.dtype != torch.float32 or split_out.dtype != torch.float16 or split_inv.dtype != torch.float32:
            raise PsalmHipError("causal_attention_split: float32 qkv buffer, float16 split buffer, float32 scales")
        self.lib.psalm_causal_attention_f32_workspace.restype = c_long
        nbytes = self.lib.psalm_causal_attention_f32_workspace(B, L, heads)
        key = ("causal_f32_ws", nbytes)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        rc = self.lib.psalm_causal_attention_f32_split(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._p(split_out),
                                                       c_long(split_out.stride(0)), split_out.shape[1] // 2, split_col_off,
                                                       self._p(split_inv), self._p(cos), self._p(sin), self._p(key_mask), self._p(ws),
                                                       B, L, heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_causal_attention_f32_split")
        return split_out

    # ---- prefix form (image sessions): suffix rows of N prompts against one cached prefix, see psalm_causal_attention_f32_prefix
    def _prefix_attn_ws(self, N, S, heads):
        self.lib.psalm_causal_attention_f32_prefix_workspace.restype = c_long
        nbytes = self.lib.psalm_causal_attention_f32_prefix_workspace(N, S, heads)
        key = ("causal_prefix_ws", nbytes)         # (as causal_f32_ws: one per binding -- a binding serves one stream at a time, PSALM.replica)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    @staticmethod
    def _check_prefix_cache(k_cache, v_cache, P, heads):
        Pp = (P + 31) // 32 * 32
        if (k_cache.dtype != torch.float32 or v_cache.dtype != torch.float32 or not k_cache.is_contiguous() or k_cache.numel() != heads * Pp * 64
                or v_cache.dim() != 2 or v_cache.shape[0] != P or v_cache.shape[1] < heads * 64 or v_cache.stride(1) != 1):
            raise PsalmHipError("prefix cache: K (heads, ceil32(P), 64) float32 contiguous, V (P, >= heads*64) float32 rows")

    def phi_prefix_kv_store(self, buf, k_off, v_off, cos, sin, k_cache, v_cache, P, heads, head_dim, rot):
        """One layer's prefix cache from the [k|v|q|..] buffer of the P prefix rows: k_cache <- RoPE(k) as (heads, ceil32(P), 64), v_cache <- v rows."""
        if buf.dtype != torch.float32 or buf.shape[0] < P:
            raise PsalmHipError("phi_prefix_kv_store: float32 buffer of >= P rows")
        self._check_prefix_cache(k_cache, v_cache, P, heads)
        rc = self.lib.psalm_phi_prefix_kv_store(self._pv(buf), c_long(buf.stride(0)), k_off, v_off, self._p(cos), self._p(sin), self._p(k_cache),
                                                self._pv(v_cache), c_long(v_cache.stride(0)), P, heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_phi_prefix_kv_store")

    def causal_attention_prefix(self, buf, q_off, k_off, v_off, k_cache, v_cache, out, o_off, cos, sin, key_mask, N, S, P, heads, head_dim, rot):
        """buf (N*S, ld) float32 holds the suffix rows' q|k|v column blocks; k_cache / v_cache: the shared prefix of P rows; cos / sin (>= P+S, rot);
        key_mask (N, S) u8.  out (N*S, ldo) float32 receives the attention output at column o_off (may be `buf`: q is read before it is written)."""
        if buf.dtype != torch.float32 or out.dtype != torch.float32 or cos.shape[0] < P + S or key_mask.numel() != N * S:
            raise PsalmHipError("causal_attention_prefix: float32 buffers, cos / sin tables of >= P + S rows, key_mask (N, S)")
        self._check_prefix_cache(k_cache, v_cache, P, heads)
        ws = self._prefix_attn_ws(N, S, heads)
        rc = self.lib.psalm_causal_attention_f32_prefix(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._p(k_cache),
                                                        self._pv(v_cache), c_long(v_cache.stride(0)), self._pv(out), c_long(out.stride(0)), o_off,
                                                        self._p(cos), self._p(sin), self._p(key_mask), self._p(ws), N, S, P, heads, head_dim, rot,
                                                        self._stream())
        self._check(rc, "psalm_causal_attention_f32_prefix")
        return out

    def causal_attention_prefix_split(self, buf, q_off, k_off, v_off, k_cache, v_cache, split_out, split_inv, split_col_off, cos, sin, key_mask,
                                      N, S, P, heads, head_dim, rot):
        """causal_attention_prefix whose output goes, in split-f16 form under the row scales 1/split_inv, into columns split_col_off.. of
        `split_out` ((N*S, 2*Kp) float16; lo part Kp columns further)."""
        if (buf.dtype != torch.float32 or split_out.dtype != torch.float16 or split_inv.dtype != torch.float32 or cos.shape[0] < P + S
                or key_mask.numel() != N * S):
            raise PsalmHipError("causal_attention_prefix_split: float32 qkv buffer, float16 split buffer, float32 scales, tables of >= P + S rows")
        self._check_prefix_cache(k_cache, v_cache, P, heads)
        ws = self._prefix_attn_ws(N, S, heads)
        rc = self.lib.psalm_causal_attention_f32_prefix_split(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off, self._p(k_cache),
                                                              self._pv(v_cache), c_long(v_cache.stride(0)), self._p(split_out),
                                                              c_long(split_out.stride(0)), split_out.shape[1] // 2, split_col_off,
                                                              self._p(split_inv), self._p(cos), self._p(sin), self._p(key_mask), self._p(ws),
                                                              N, S, P, heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_causal_attention_f32_prefix_split")
        return split_out

    # ---- grouped prefix form (PSALM.segment_many): every prompt names its own prefix cache, see psalm_causal_attention_f32_prefix_grouped
    PREFIX_REF = np.dtype([("k_cache", "<u8"), ("v_cache", "<u8"), ("ldv", "<i8"), ("P", "<i4"), ("pad", "<i4")])        # psalm_prefix_ref

    def prefix_ref_table(self, caches, prompt_cache, layers=None):
        """The psalm_prefix_ref table of one grouped call as a HOST array of PREFIX_REF records, shape (len(layers), N): `caches` are (buf, views)
        pairs of phi_prefix_cache (one per session), `prompt_cache[n]` the index into `caches` of prompt n, `layers` the layer indices (default:
        all).  The caller puts it into its packed blob (or hands it to the grouped calls, which upload it) and keeps the caches alive."""
        if not len(caches) or not len(prompt_cache):
            raise PsalmHipError("prefix_ref_table: at least one cache and one prompt")
        layers = range(len(caches[0][1])) if layers is None else layers
        per = np.zeros((len(layers), len(caches)), self.PREFIX_REF)
        for c, (_, views) in enumerate(caches):
            for j, i in enumerate(layers):
                kc, vc = views[i]
                if kc.dtype != torch.float32 or vc.dtype != torch.float32 or not kc.is_contiguous() or vc.dim() != 2 or vc.stride(1) != 1 \
                        or kc.dim() != 3 or kc.shape[1] != (vc.shape[0] + 31) // 32 * 32 or kc.shape[2] != 64 or vc.shape[1] < kc.shape[0] * 64:
                    raise PsalmHipError("prefix cache: K (heads, ceil32(P), 64) float32 contiguous, V (P, >= heads*64) float32 rows")
                per[j, c] = (kc.data_ptr(), vc.data_ptr(), vc.stride(0), vc.shape[0], 0)
        idx = np.asarray(prompt_cache, np.int64)
        if idx.min() < 0 or idx.max() >= len(caches):
            raise PsalmHipError("prefix_ref_table: prompt_cache indexes `caches`")
        return np.ascontiguousarray(per[:, idx])

    def _prefix_refs(self, refs, table, n, P_max, heads, name):
        """the device bytes of a table (uploading a host one); whatever host copy is at hand is checked against n entries, P_max and the entry rules"""
        if isinstance(refs, np.ndarray):
            table = refs
            t = np.ascontiguousarray(refs)
            refs = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).to(self.device)
        if table is not None:
            t = np.asarray(table)
            if t.dtype != self.PREFIX_REF or t.size != n:
                raise PsalmHipError(f"{name}: a table of {n} PREFIX_REF entries")
            if (t["P"] < 1).any() or int(t["P"].max()) > P_max:
                raise PsalmHipError(f"{name}: every table entry needs 1 <= P <= P_max = {P_max}")
            if (t["k_cache"] == 0).any() or (t["v_cache"] == 0).any() or (t["k_cache"] % 16).any() or (t["v_cache"] % 16).any() \
                    or (t["ldv"] < heads * 64).any() or (t["ldv"] % 4).any() or ((t["P"].astype(np.int64) - 1) * t["ldv"] * 4 + 256 >= 0x7fffffff).any():
                raise PsalmHipError(f"{name}: table entries need 16-byte aligned caches, V rows of ldv >= heads * 64 floats, P * ldv * 4 below 2 GiB")
        if refs is not None and (refs.dtype != torch.uint8 or refs.numel() != 32 * n or not refs.is_contiguous() or refs.data_ptr() % 16):
            raise PsalmHipError(f"{name}: the device table is {n} x 32 contiguous bytes, 16-byte aligned")
        return refs

    def causal_attention_prefix_grouped(self, buf, q_off, k_off, v_off, refs, out, o_off, cos, sin, key_mask, N, S, P_max, heads, head_dim, rot,
                                        table=None):
        """causal_attention_prefix with one prefix per prompt: `refs` is the (N) table of prefix_ref_table (one layer), as a host array (uploaded here)
        or as device bytes (then `table` may carry its host copy for the checks); cos / sin (>= P_max + S, rot)."""
        if buf.dtype != torch.float32 or out.dtype != torch.float32 or cos.shape[0] < P_max + S or key_mask.numel() != N * S:
            raise PsalmHipError("causal_attention_prefix_grouped: float32 buffers, cos / sin tables of >= P_max + S rows, key_mask (N, S)")
        refs = self._prefix_refs(refs, table, N, P_max, heads, "causal_attention_prefix_grouped")
        ws = self._prefix_attn_ws(N, S, heads)
        rc = self.lib.psalm_causal_attention_f32_prefix_grouped(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off,
                                                                self._p(refs) if refs is not None else None, P_max, self._pv(out),
                                                                c_long(out.stride(0)), o_off, self._p(cos), self._p(sin), self._p(key_mask),
                                                                self._p(ws), N, S, heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_causal_attention_f32_prefix_grouped")
        return out

    def causal_attention_prefix_grouped_split(self, buf, q_off, k_off, v_off, refs, split_out, split_inv, split_col_off, cos, sin, key_mask,
                                              N, S, P_max, heads, head_dim, rot, table=None):
        """causal_attention_prefix_grouped whose output leaves as causal_attention_prefix_split's does"""
        if (buf.dtype != torch.float32 or split_out.dtype != torch.float16 or split_inv.dtype != torch.float32 or cos.shape[0] < P_max + S
                or key_mask.numel() != N * S):
            raise PsalmHipError("causal_attention_prefix_grouped_split: float32 qkv buffer, float16 split buffer, float32 scales, tables of >= P_max + S rows")
        refs = self._prefix_refs(refs, table, N, P_max, heads, "causal_attention_prefix_grouped_split")
        ws = self._prefix_attn_ws(N, S, heads)
        rc = self.lib.psalm_causal_attention_f32_prefix_grouped_split(self._pv(buf), c_long(buf.stride(0)), q_off, k_off, v_off,
                                                                      self._p(refs) if refs is not None else None, P_max, self._p(split_out),
                                                                      c_long(split_out.stride(0)), split_out.shape[1] // 2, split_col_off,
                                                                      self._p(split_inv), self._p(cos), self._p(sin), self._p(key_mask),
                                                                      self._p(ws), N, S, heads, head_dim, rot, self._stream())
        self._check(rc, "psalm_causal_attention_f32_prefix_grouped_split")
        return split_out

    def mha_attention(self, q, k, v, B, Lq, Lk, heads, mask=None, row_all_masked=None, workspace=None):
        """q (B*Lq, D) / k, v (B*Lk, D) row-strided views, head_dim 32; mask (B,Lq,Lk) u8 1 = blocked.  workspace: a caller's uint8 buffer for the
        fp32 kernel's partial states (psalm_mha_attention_f32_workspace bytes) instead of the binding's cached one."""
        D = heads * 32
        out = self.empty(B * Lq, D, dtype=q.dtype)
        if q.dtype == torch.float32 and Lq <= 128 and all(t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (q, k, v)):
            self.lib.psalm_mha_attention_f32_workspace.restype = c_long          # fp32 matrix-core kernel, split over 256-key chunks
            nbytes = self.lib.psalm_mha_attention_f32_workspace(B, heads, Lq, Lk)
            ws = None
            if nbytes and workspace is not None:
                if workspace.dtype != torch.uint8 or workspace.numel() < nbytes:
                    raise PsalmHipError(f"mha_attention: workspace of >= {nbytes} bytes (uint8)")
                ws = workspace
            elif nbytes:
                key = ("mha_f32_ws", nbytes)
                ws = self._ws.get(key)
                if ws is None:
                    ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            rc = self.lib.psalm_mha_attention_f32(self._pv(q), c_long(q.stride(0)), self._pv(k), c_long(k.stride(0)), self._pv(v),
                                                  c_long(v.stride(0)), self._p(out), c_long(D), self._p(mask), self._p(row_all_masked),
                                                  self._p(ws), B, Lq, Lk, heads, 32, self._stream())
            self._check(rc, "psalm_mha_attention_f32")
            return out
        rc = self.lib.psalm_mha_attention(self._pv(q), c_long(q.stride(0)), self._pv(k), c_long(k.stride(0)), self._pv(v),
                                          c_long(v.stride(0)), self._p(out), c_long(D), _dt(q), self._p(mask),
                                          self._p(row_all_masked), B, Lq, Lk, heads, 32, self._stream())
        self._check(rc, "psalm_mha_attention")
        return out

    def mha_attention_f32_shared_workspace(self, B, heads, Lq, Lk):
        self.lib.psalm_mha_attention_f32_shared_workspace.restype = c_long
        return int(self.lib.psalm_mha_attention_f32_shared_workspace(B, heads, Lq, Lk))

    def mha_attention_f32_shared(self, q, k, v, B, Lq, Lk, heads, mask=None, row_all_masked=None, workspace=None):
        """B query sets against ONE K / V (psalm_mha_attention_f32_shared): q (B*Lq, D), k / v (Lk, D) row-strided float32 views, mask (B, Lq, Lk) u8
        1 = blocked, row_all_masked (B*Lq) u8.  Set b's words are those of mha_attention(B = 1) on it alone.  workspace: as mha_attention's."""
        D = heads * 32
        if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32 or q.shape[0] != B * Lq or k.shape[0] != Lk or v.shape[0] != Lk:
            raise PsalmHipError("mha_attention_f32_shared: float32 q (B*Lq, D), k / v (Lk, D)")
        out = self.empty(B * Lq, D, dtype=torch.float32)
        nbytes = self.mha_attention_f32_shared_workspace(B, heads, Lq, Lk)
        ws = None
        if nbytes and workspace is not None:
            if workspace.dtype != torch.uint8 or workspace.numel() < nbytes:
                raise PsalmHipError(f"mha_attention_f32_shared: workspace of >= {nbytes} bytes (uint8)")
            ws = workspace
        elif nbytes:
            ws = self._stage_ws("mha_f32_shared", nbytes)
        rc = self.lib.psalm_mha_attention_f32_shared(self._pv(q), c_long(q.stride(0)), self._pv(k), c_long(k.stride(0)), self._pv(v),
                                                     c_long(v.stride(0)), self._p(out), c_long(D), self._p(mask), self._p(row_all_masked),
                                                     self._p(ws), B, Lq, Lk, heads, 32, self._stream())
        self._check(rc, "psalm_mha_attention_f32_shared")
        return out

    def mha_attention_t(self, q, k, vt, B, Lq, Lk, heads, mask=None, row_all_masked=None):
        """Matrix-core split-KV form: q (B*Lq, D) / k (B*Lk, D) row-strided bf16 views; vt (B*D, ldvt) = V transposed
        (row h*32+d, columns = keys, zero padded).  mask (B,Lq,Lk) u8 1 = blocked."""
        D = heads * 32
        out = self.empty(B * Lq, D, dtype=torch.bfloat16)
        self.lib.psalm_mha_attention_mfma_workspace.restype = c_long
        nbytes = self.lib.psalm_mha_attention_mfma_workspace(B, heads, Lk)
        ws = None
        if nbytes:
            key = ("mha_ws", nbytes)
            ws = self._ws.get(key)
            if ws is None:
                ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        rc = self.lib.psalm_mha_attention_mfma(self._pv(q), c_long(q.stride(0)), self._pv(k), c_long(k.stride(0)), self._pv(vt),
                                               c_long(vt.stride(0)), self._p(out), c_long(D), self._p(mask), self._p(row_all_masked),
                                               self._p(ws), B, Lq, Lk, heads, 32, self._stream())
        self._check(rc, "psalm_mha_attention_mfma")
        return out

    def attn_mask(self, masks, Ht, Wt):
        """masks (B,Q,h,w) f32 logits -> (u8 (B,Q,Ht*Wt) 1 = blocked, u8 (B,Q) all-masked flags)."""
        B, Q, h, w = masks.shape
        out = self.empty(B, Q, Ht * Wt, dtype=torch.uint8)
        flags = self.empty(B, Q, dtype=torch.uint8)
        rc = self.lib.psalm_attn_mask(self._p(masks), self._p(out), self._p(flags), B * Q, h, w, Ht, Wt, self._stream())
        self._check(rc, "psalm_attn_mask")
        return out, flags

    # ------------------------------------------------------------------ image / layout ops
    def patch_im2col(self, img, ps, Kpad, out_dtype=torch.float32):
        B, Cin, H, W = img.shape
        Hp, Wp = (H + ps - 1) // ps, (W + ps - 1) // ps
        out = self.empty(B * Hp * Wp, Kpad, dtype=out_dtype)
        rc = self.lib.psalm_patch_im2col(self._p(img), self._p(out), _dt(out), B, Cin, H, W, ps, Kpad, self._stream())
        self._check(rc, "psalm_patch_im2col")
        return out

    def image_preprocess(self, img, nh, nw, S, mean, std):
        """img (H,W,3) uint8 RGB on the device -> (image (3,S,S) float32 normalised, padding_mask (S,S) bool): Pillow-bilinear resize to
        (nh, nw) (bit-identical to PIL / detectron2 ResizeShortestEdge), pad bottom/right with 128, (x - mean) / std."""
        from .preprocess import pil_bilinear_tables
        if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
            raise PsalmHipError("image_preprocess: (H,W,3) uint8 image expected")
        H, W = int(img.shape[0]), int(img.shape[1])
        key = ("pp_tables", H, W, nh, nw)
        tb = self._ws.get(key)
        if tb is None:
            if len([k for k in self._ws if isinstance(k, tuple) and k[0] == "pp_tables"]) > 64:
                for k in [k for k in self._ws if isinstance(k, tuple) and k[0] == "pp_tables"]:
                    del self._ws[k]
            bh, kh, ksh = pil_bilinear_tables(W, nw) if nw != W else (None, None, 0)
            bv, kv, ksv = pil_bilinear_tables(H, nh) if nh != H else (None, None, 0)
            dev = lambda a: torch.from_numpy(a).to(self.device) if a is not None else None
            tb = self._ws[key] = (dev(bh), dev(kh), ksh, dev(bv), dev(kv), ksv)
        bh, kh, ksh, bv, kv, ksv = tb
        out = self.empty(3, S, S, dtype=torch.float32)
        pm = self.empty(S, S, dtype=torch.uint8)
        tmp = self.empty(H * nw * 3, dtype=torch.uint8) if nw != W else None
        m = (c_float * 3)(*[float(v) for v in mean.reshape(-1)])
        d = (c_float * 3)(*[float(v) for v in std.reshape(-1)])
        rc = self.lib.psalm_image_preprocess(self._p(img), H, W, self._p(out), self._p(pm), S, nh, nw, self._p(bh), self._p(kh), ksh,
                                             self._p(bv), self._p(kv), ksv, self._p(tmp), m, d, self._stream())
        self._check(rc, "psalm_image_preprocess")
        return out, pm.view(torch.bool)

    def im2col_nhwc(self, x, B, H, W, k, stride, pad):
        C = x.shape[-1]
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out = self.empty(B * Ho * Wo, k * k * C, dtype=x.dtype)
        rc = self.lib.psalm_im2col_nhwc(self._p(x), self._p(out), _dt(x), B, H, W, C, k, stride, pad, self._stream())
        self._check(rc, "psalm_im2col_nhwc")
        return out

    def im2col_split(self, x, B, H, W, k, stride, pad):
        """im2col_nhwc + split_f16 in one pass: x (B*H*W, C) float32 NHWC tokens -> SplitF16 of the (B*Ho*Wo, k*k*C) patch matrix."""
        C = x.shape[-1]
        if x.dtype != torch.float32 or C % 8:
            raise PsalmHipError("im2col_split: float32 input, C % 8 == 0")
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        K = k * k * C
        Kp = (K + 63) // 64 * 64
        t = self.empty(B * Ho * Wo, 2 * Kp, dtype=torch.float16)
        inv = self.empty(B * Ho * Wo, dtype=torch.float32)
        rc = self.lib.psalm_im2col_split_f16(self._p(x), self._p(t), self._p(inv), B, H, W, C, k, stride, pad, self._stream())
        self._check(rc, "psalm_im2col_split_f16")
        return SplitF16(t, inv, K)

    def resize_planes(self, x, H, W, crop=None, out_dtype=None, out=None):
        """x (N,h,w) -> bilinear (align_corners=False) -> (N,H,W); optional crop (hc,wc) of the input first.  `out`: a contiguous (N,H,W)
        buffer to write into (tests use a view that is not 16-byte aligned to reach the one-pixel-per-thread kernel)."""
        N, h, w = x.shape
        hc, wc = crop if crop is not None else (h, w)
        if out is None:
            out = self.empty(N, H, W, dtype=out_dtype or x.dtype)
        elif tuple(out.shape) != (N, H, W) or not out.is_contiguous():
            raise PsalmHipError("resize_planes: out must be a contiguous (N, H, W) tensor")
        rc = self.lib.psalm_resize_planes(self._p(x), _dt(x), self._p(out), _dt(out), c_long(N), h, w, hc, wc, H, W, self._stream())
        self._check(rc, "psalm_resize_planes")
        return out

    def upsample_add_nhwc(self, lateral, small, B, h, w, H, W, out_dtype=None):
        C = lateral.shape[-1]
        out = self.empty(B * H * W, C, dtype=out_dtype or lateral.dtype)
        rc = self.lib.psalm_upsample_add_nhwc(self._p(lateral), _dt(lateral), self._p(small), _dt(small), self._p(out), _dt(out), B, h,
                                              w, H, W, C, self._stream())
        self._check(rc, "psalm_upsample_add_nhwc")
        return out

    def region_pool(self, tokens, img_of_region, pts, h, w, n_img):
        """tokens (B*h*w, C) f32; img_of_region (R,) i32; pts (R,n,2) f32 (y,x) -> (R, C) f32."""
        R, n = pts.shape[0], pts.shape[1]
        C = tokens.shape[-1]
        out = self.empty(R, C, dtype=torch.float32)
        if tokens.dtype != torch.float32:
            raise PsalmHipError("region_pool expects fp32 image tokens")
        rc = self.lib.psalm_region_pool(self._p(tokens), self._p(img_of_region), self._p(pts), self._p(out), R, h, w, C, n,
                                        self._stream())
        self._check(rc, "psalm_region_pool")
        return out

    def permute_layout(self, x, B, C, HW, to_nhwc, out_dtype=None):
        out = self.empty((B * HW, C) if to_nhwc else (B, C, HW), dtype=out_dtype or x.dtype)
        rc = self.lib.psalm_permute_layout(self._p(x), _dt(x), self._p(out), _dt(out), B, C, c_long(HW), int(to_nhwc), self._stream())
        self._check(rc, "psalm_permute_layout")
        return out

    # ------------------------------------------------------------------ post-processing
    def class_softmax(self, cls, Kpad, probsT_dtype=torch.float32):
        """cls (Q,C1) f32 -> probs (Q,C1), probsT (C1-1,Kpad) zero padded, score (Q), label (Q) i32."""
        Q, C1 = cls.shape
        probs = self.empty(Q, C1)
        probsT = self.zeros(C1 - 1, Kpad, dtype=probsT_dtype)
        score = self.empty(Q)
        label = self.empty(Q, dtype=torch.int32)
        rc = self.lib.psalm_class_softmax(self._p(cls), self._p(probs), self._p(probsT), _dt(probsT), self._p(score), self._p(label),
                                          Q, C1, Kpad, self._stream())
        self._check(rc, "psalm_class_softmax")
        return probs, probsT, score, label

    def sigmoid_transpose(self, mask, Kpad, out_dtype):
        """mask (Q,HW) f32 -> (HW,Kpad) sigmoid, zero padded."""
        Q, HW = mask.shape
        out = self.empty(HW, Kpad, dtype=out_dtype)
        rc = self.lib.psalm_sigmoid_transpose(self._p(mask), self._p(out), _dt(out), Q, c_long(HW), Kpad, self._stream())
        self._check(rc, "psalm_sigmoid_transpose")
        return out

    def semantic_from_masks(self, mask, probsT, want_mask_score=False):
        """mask (Q,HW) f32 logits, probsT (C,128) bf16 -> (C,HW) f32 = probsT @ sigmoid(mask), one pass over the logits; with
        want_mask_score also returns mask_scores(mask) accumulated from the same read."""
        Q, HW = mask.shape
        C, Kpad = probsT.shape
        if probsT.dtype not in (torch.bfloat16, torch.float32) or mask.dtype != torch.float32:
            raise PsalmHipError("semantic_from_masks: f32 logits, bf16 probsT (bf16 MFMA) or f32 probsT (split-f16, fp32-class)")
        out = self.empty(C, HW, dtype=torch.float32)
        ms = self.empty(Q) if want_mask_score else None
        ws = self.empty(Q * 512 * 2) if want_mask_score else None
        fn = self.lib.psalm_semantic_from_masks_x3 if probsT.dtype == torch.float32 else self.lib.psalm_semantic_from_masks
        rc = fn(self._p(mask), self._p(probsT), self._p(out), self._p(ms) if want_mask_score else None,
                self._p(ws) if want_mask_score else None, Q, C, c_long(HW), Kpad, self._stream())
        self._check(rc, "psalm_semantic_from_masks")
        return (out, ms) if want_mask_score else out

    def mask_scores(self, mask):
        """mask (Q,HW) f32 -> (Q) f32: sum(sigmoid*[m>0]) / (sum([m>0]) + 1e-6)."""
        Q, HW = mask.shape
        score = self.empty(Q)
        ws = self.empty(Q * 64 * 2)
        rc = self.lib.psalm_mask_scores(self._p(mask), self._p(score), self._p(ws), Q, c_long(HW), self._stream())
        self._check(rc, "psalm_mask_scores")
        return score

    def topk_select(self, vals, C, k, is_thing=None, mask_score=None, apply_sigmoid=False, count_out=None):
        """vals (Q,stride) f32, first C columns are candidates.  Returns (score (k), class (k) i32, query (k) i32, count (1) i32),
        entries [0,count) valid, in descending candidate order.  count_out: a zeroed (1,) int32 view to write the count into."""
        Q, stride = vals.shape
        sc = self.zeros(k)
        cl = self.zeros(k, dtype=torch.int32)
        qq = self.zeros(k, dtype=torch.int32)
        cnt = count_out if count_out is not None else self.zeros(1, dtype=torch.int32)
        rc = self.lib.psalm_topk_select(self._p(vals), Q, C, stride, k, self._p(is_thing), self._p(mask_score), self._p(sc), self._p(cl),
                                        self._p(qq), self._p(cnt), int(apply_sigmoid), self._stream())
        self._check(rc, "psalm_topk_select")
        return sc, cl, qq, cnt

    def binarize_gather(self, mask, n, query=None, count=None):
        """out[i] = (mask[query[i]] > 0).float() for i < count (rows >= count untouched); mask (Q,H,W)."""
        Q, Hh, Ww = mask.shape
        out = self.empty(n, Hh, Ww)
        rc = self.lib.psalm_binarize_gather(self._p(mask), self._p(query), self._p(count), self._p(out), n, c_long(Hh * Ww), self._stream())
        self._check(rc, "psalm_binarize_gather")
        return out

    def panoptic(self, mask, score, label, is_thing, num_classes, obj_thr, overlap_thr, info_out=None, ninfo_out=None):
        """mask (Q,H,W) f32 logits; returns (pan (H,W) i32, info (Q,3) i32, ninfo (1) i32).  info_out / ninfo_out: zeroed int32 views
        ((Q,3) / (1,)) to write into -- the caller fetches its data-dependent counts in ONE device-to-host copy."""
        Q, Hh, Ww = mask.shape
        HW = Hh * Ww
        argq = self.empty(HW, dtype=torch.int32)
        counts = self.empty(Q * 3, dtype=torch.int32)
        final_id = self.empty(Q + num_classes + 1, dtype=torch.int32)
        pan = self.empty(Hh, Ww, dtype=torch.int32)
        info = info_out if info_out is not None else self.zeros(Q, 3, dtype=torch.int32)
        ninfo = ninfo_out if ninfo_out is not None else self.zeros(1, dtype=torch.int32)
        rc = self.lib.psalm_panoptic(self._p(mask), self._p(score), self._p(label), self._p(is_thing), self._p(argq), self._p(counts),
                                     self._p(final_id), self._p(pan), self._p(info), self._p(ninfo), Q, c_long(HW), num_classes,
                                     c_float(obj_thr), c_float(overlap_thr), self._stream())
        self._check(rc, "psalm_panoptic")
        return pan, info, ninfo

    def region_scores(self, logits, mask_score):
        """logits (K,Q) f32 -> (Q,K) sigmoid(logits).T * mask_score[:,None]."""
        K, Q = logits.shape
        out = self.empty(Q, K)
        rc = self.lib.psalm_region_scores(self._p(logits), self._p(mask_score), self._p(out), K, Q, self._stream())
        self._check(rc, "psalm_region_scores")
        return out

    # ------------------------------------------------------------------ MSDA
    def msda_forward(self, value, spatial_shapes: Sequence[Sequence[int]], level_start: Sequence[int], loc, attw,
                     out_dtype=None):
        """value (B,S,M,D); loc (B,Lq,M,L,P,2) f32; attw (B,Lq,M,L,P) f32 -> (B,Lq,M*D).
        Contract of the reference op MSDA.ms_deform_attn_forward (ops/src/ms_deform_attn.h:25-44)."""
        B, S, M, D = value.shape
        _, Lq, _, L, P, _ = loc.shape
        if loc.dtype != torch.float32 or attw.dtype != torch.float32:
            raise PsalmHipError("sampling locations / attention weights must be float32")
        out = self.empty(B, Lq, M * D, dtype=out_dtype or value.dtype)
        sh = (ctypes.c_int64 * (2 * L))(*[int(x) for hw in spatial_shapes for x in hw])
        st = (ctypes.c_int64 * L)(*[int(x) for x in level_start])
        rc = self.lib.psalm_msda_forward(self._p(value), _dt(value), sh, st, self._p(loc), self._p(attw), self._p(out),
                                         _dt(out), B, S, M, D, L, Lq, P, self._stream())
        self._check(rc, "psalm_msda_forward")
        return out

    def msda_forward_dev(self, value, spatial_shapes, level_start, loc, attw, out_dtype=None):
        """msda_forward with `spatial_shapes` (L,2) / `level_start` (L) as int64 tensors ON THE DEVICE (the reference op's signature):
        nothing is copied to the host, the call is asynchronous."""
        B, S, M, D = value.shape
        _, Lq, _, L, P, _ = loc.shape
        for t in (spatial_shapes, level_start):
            if t.dtype != torch.int64 or t.device != value.device:
                raise PsalmHipError("msda_forward_dev: int64 level tensors on the value's device")
        if tuple(spatial_shapes.shape) != (L, 2) or level_start.numel() != L:
            raise PsalmHipError(f"msda_forward_dev: level table shapes {tuple(spatial_shapes.shape)} / {tuple(level_start.shape)} for L = {L}")
        # each DISTINCT level table is checked against S once (one small D2H copy the first time; keyed by storage + version counter, so
        # the steady state stays asynchronous); not during stream capture, where the kernel's own bounds guard is the safety net
        key = (spatial_shapes.data_ptr(), spatial_shapes._version, level_start.data_ptr(), level_start._version, S, L)
        if key not in self._msda_tables and not (value.is_cuda and torch.cuda.is_current_stream_capturing()):
            hw, st = spatial_shapes.cpu().tolist(), level_start.reshape(-1).cpu().tolist()
            if any(h <= 0 or w_ <= 0 or s0 < 0 or s0 + h * w_ > S for (h, w_), s0 in zip(hw, st)) or sum(h * w_ for h, w_ in hw) != S:
                raise PsalmHipError(f"msda_forward_dev: level table {hw} / starts {st} does not describe the {S} rows of value")
            if len(self._msda_tables) > 64:
                self._msda_tables.clear()
            self._msda_tables.add(key)
        out = self.empty(B, Lq, M * D, dtype=out_dtype or value.dtype)
        rc = self.lib.psalm_msda_forward_dev(self._p(value), _dt(value), self._p(spatial_shapes.contiguous()), self._p(level_start.contiguous()),
                                             self._p(loc), self._p(attw), self._p(out), _dt(out), B, S, M, D, L, Lq, P, self._stream())
        self._check(rc, "psalm_msda_forward_dev")
        return out

    def msda_policy(self, v: int):
        """psalm_msda_set_policy: 1 (default) / 0 = quad-shared bilinear taps on / off (A/B runs, tests)"""
        self._check(self._cdll_raw.psalm_msda_set_policy(int(v)), "psalm_msda_set_policy")

    def msda_fused(self, value, spatial_shapes, level_start, offsets_logits, M, out_dtype=None):
        """value (B,S,M*D); offsets_logits (B,S,M*L*P*3) f32 = [offsets | logits] -> (B,S,M*D)."""
        B, S, C = value.shape
        L, P = len(spatial_shapes), 4
        D = C // M
        if offsets_logits.dtype != torch.float32 or offsets_logits.shape[-1] != M * L * P * 3:
            raise PsalmHipError("offsets_logits must be float32 (B,S,M*L*P*3)")
        out = self.empty(B, S, C, dtype=out_dtype or value.dtype)
        sh = (ctypes.c_int64 * (2 * L))(*[int(x) for hw in spatial_shapes for x in hw])
        st = (ctypes.c_int64 * L)(*[int(x) for x in level_start])
        rc = self.lib.psalm_msda_fused(self._p(value), _dt(value), sh, st, self._p(offsets_logits), self._p(out), _dt(out),
                                       B, S, M, D, L, P, self._stream())
        self._check(rc, "psalm_msda_fused")
        return out


    # ------------------------------------------------------------------ video object tracking (csrc/video.hip)
    @staticmethod
    def _want(t, dtype, shape, what):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise PsalmHipError(f"{what}: contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        return t

    def video_pick(self, scores, pick_query=None, pick_score=None):
        """scores (Q,R) f32 -> (pick_query (R) i32, pick_score (R) f32): psalm_video_pick (eval_davis.py:443-457).  The outputs may be given
        (views of a caller-owned block)."""
        if scores.dim() != 2 or scores.dtype != torch.float32:
            raise PsalmHipError("video_pick: scores (Q,R) float32")
        Q, R = scores.shape
        pick_query = self.empty(R, dtype=torch.int32) if pick_query is None else self._want(pick_query, torch.int32, (R,), "video_pick pick_query")
        pick_score = self.empty(R, dtype=torch.float32) if pick_score is None else self._want(pick_score, torch.float32, (R,), "video_pick pick_score")
        self._check(self.lib.psalm_video_pick(self._p(scores), Q, R, self._p(pick_query), self._p(pick_score), self._stream()), "psalm_video_pick")
        return pick_query, pick_score

    def video_fuse(self, pred_masks, pick_query, fill, inter=None, union=None, nonzero=None, flag=None):
        """pred_masks (Q,H,W) f32 of 0 / 1, pick_query (R) i32, fill (R) i32 -> picked (R,H,W) u8, fused (H,W) u8, inter (R,R) i32, union (R,R) i32,
        nonzero (R) i32, flag (1) i32: psalm_video_fuse.  The four count outputs may be given (views of a caller-owned block)."""
        if pred_masks.dim() != 3 or pred_masks.dtype != torch.float32:
            raise PsalmHipError("video_fuse: pred_masks (Q,H,W) float32")
        Q, Hh, Ww = pred_masks.shape
        R = int(pick_query.numel())
        self._want(pick_query, torch.int32, (R,), "video_fuse pick_query")
        self._want(fill, torch.int32, (R,), "video_fuse fill")
        inter = self.empty(R, R, dtype=torch.int32) if inter is None else self._want(inter, torch.int32, (R, R), "video_fuse inter")
        union = self.empty(R, R, dtype=torch.int32) if union is None else self._want(union, torch.int32, (R, R), "video_fuse union")
        nonzero = self.empty(R, dtype=torch.int32) if nonzero is None else self._want(nonzero, torch.int32, (R,), "video_fuse nonzero")
        flag = self.empty(1, dtype=torch.int32) if flag is None else self._want(flag, torch.int32, (1,), "video_fuse flag")
        self.lib.psalm_video_fuse_workspace.restype = c_long
        nbytes = self.lib.psalm_video_fuse_workspace(R)
        if nbytes < 0:
            raise PsalmHipError(f"video_fuse: {R} objects (1..32)")
        ws = self._stage_ws("video_fuse", nbytes)
        picked = self.empty(R, Hh, Ww, dtype=torch.uint8)
        fused = self.empty(Hh, Ww, dtype=torch.uint8)
        rc = self.lib.psalm_video_fuse(self._p(pred_masks), self._p(pick_query), self._p(fill), Q, R, c_long(Hh * Ww), self._p(picked), self._p(fused),
                                       self._p(inter), self._p(union), self._p(nonzero), self._p(flag), self._p(ws), c_long(nbytes), self._stream())
        self._check(rc, "psalm_video_fuse")
        return picked, fused, inter, union, nonzero, flag

    def mask_resize_nearest_pad(self, masks, row_tab, col_tab, total=None):
        """masks (R,h,w) u8, row_tab (Sh) / col_tab (Sw) i32 source indices (-1 = pad) -> (out (R,Sh,Sw) u8, row_cnt (R,Sh) i32); total (R) i32:
        a ZEROED buffer that receives the non-zero pixels per mask.  psalm_mask_resize_nearest_pad."""
        if masks.dim() != 3 or masks.dtype != torch.uint8:
            raise PsalmHipError("mask_resize_nearest_pad: masks (R,h,w) uint8")
        R, h, w = masks.shape
        Sh, Sw = int(row_tab.numel()), int(col_tab.numel())
        self._want(row_tab, torch.int32, (Sh,), "mask_resize_nearest_pad row_tab")
        self._want(col_tab, torch.int32, (Sw,), "mask_resize_nearest_pad col_tab")
        if total is not None:
            self._want(total, torch.int32, (R,), "mask_resize_nearest_pad total")
        out = self.empty(R, Sh, Sw, dtype=torch.uint8)
        row_cnt = self.empty(R, Sh, dtype=torch.int32)
        rc = self.lib.psalm_mask_resize_nearest_pad(self._p(masks), R, h, w, self._p(row_tab), self._p(col_tab), Sh, Sw, self._p(out), self._p(row_cnt),
                                                    self._p(total), self._stream())
        self._check(rc, "psalm_mask_resize_nearest_pad")
        return out, row_cnt

    def mask_select_points(self, masks, row_cnt, idx):
        """masks (R,Sh,Sw) u8, row_cnt (R,Sh) i32, idx (R,n) i32 ranks in nonzero() order -> pts (R,n,2) f32 (y / Sh, x / Sw): psalm_mask_select_points."""
        if masks.dim() != 3 or masks.dtype != torch.uint8:
            raise PsalmHipError("mask_select_points: masks (R,Sh,Sw) uint8")
        R, Sh, Sw = masks.shape
        n = int(idx.shape[-1])
        self._want(row_cnt, torch.int32, (R, Sh), "mask_select_points row_cnt")
        self._want(idx, torch.int32, (R, n), "mask_select_points idx")
        pts = self.empty(R, n, 2, dtype=torch.float32)
        rc = self.lib.psalm_mask_select_points(self._p(masks), self._p(row_cnt), self._p(idx), R, Sh, Sw, n, self._p(pts), self._stream())
        self._check(rc, "psalm_mask_select_points")
        return pts

    # ------------------------------------------------------------------ region prompts of image sessions (csrc/prompts.hip)
    def mask_rasterize(self, prims, R, h, w, out=None):
        """prims (n,6) i32 rows of psalm_prompt_prim (region, kind, a, b, c, d; kind 0: pixel (a, b), kind 1: box rows [a,c) x cols [b,d)) on the
        device -> masks (R,h,w) u8, zeroed by the call: psalm_mask_rasterize."""
        n = int(prims.shape[0])
        self._want(prims, torch.int32, (n, 6), "mask_rasterize prims")
        out = self.empty(R, h, w, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (R, h, w), "mask_rasterize out")
        rc = self.lib.psalm_mask_rasterize(self._p(prims) if n else c_void_p(0), n, int(R), int(h), int(w), self._p(out), self._stream())
        self._check(rc, "psalm_mask_rasterize")
        return out

    def mask_dilate_disc(self, masks, radius, max_radius, out=None):
        """masks (R,h,w) u8, radius (R) i32 on the device (< 0: the plane is copied), 0 <= max_radius <= 16 bounding every radius -> (R,h,w) u8,
        enhance_with_circles per plane: psalm_mask_dilate_disc.  `out` must not be `masks`."""
        if masks.dim() != 3 or masks.dtype != torch.uint8:
            raise PsalmHipError("mask_dilate_disc: masks (R,h,w) uint8")
        R, h, w = masks.shape
        self._want(radius, torch.int32, (R,), "mask_dilate_disc radius")
        out = self.empty(R, h, w, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (R, h, w), "mask_dilate_disc out")
        rc = self.lib.psalm_mask_dilate_disc(self._p(masks), self._p(radius), int(max_radius), R, h, w, self._p(out), self._stream())
        self._check(rc, "psalm_mask_dilate_disc")
        return out

    def region_best(self, scores, best_query=None, best_score=None):
        """scores (Q,R) f32 -> (best_query (R) i32: first arg-max of column r, best_score (R) f32): psalm_region_best.  The outputs may be given
        (views of a caller-owned block)."""
        if scores.dim() != 2 or scores.dtype != torch.float32:
            raise PsalmHipError("region_best: scores (Q,R) float32")
        Q, R = scores.shape
        best_query = self.empty(R, dtype=torch.int32) if best_query is None else self._want(best_query, torch.int32, (R,), "region_best best_query")
        best_score = self.empty(R, dtype=torch.float32) if best_score is None else self._want(best_score, torch.float32, (R,), "region_best best_score")
        self._check(self.lib.psalm_region_best(self._p(scores), Q, R, self._p(best_query), self._p(best_score), self._stream()), "psalm_region_best")
        return best_query, best_score

    def mask_gather_u8(self, masks, query):
        """masks (Q,H,W) f32, query (R) i32 -> (R,H,W) u8 = masks[query] > 0: psalm_mask_gather_u8."""
        if masks.dim() != 3 or masks.dtype != torch.float32:
            raise PsalmHipError("mask_gather_u8: masks (Q,H,W) float32")
        Q, Hh, Ww = masks.shape
        R = int(query.numel())
        self._want(query, torch.int32, (R,), "mask_gather_u8 query")
        out = self.empty(R, Hh, Ww, dtype=torch.uint8)
        rc = self.lib.psalm_mask_gather_u8(self._p(masks), self._p(query), Q, R, c_long(Hh * Ww), self._p(out), self._stream())
        self._check(rc, "psalm_mask_gather_u8")
        return out

    # ------------------------------------------------------------------ boxes and areas from masks (csrc/maskbox.hip)
    def mask_boxes(self, masks, index=None, out_boxes=None, out_areas=None, workspace=None):
        """masks (n,H,W) float32 (set: > 0) | uint8 / bool (set: != 0) -> (boxes (m,4) f32 = (x_min, y_min, x_max + 1, y_max + 1), zeros for an empty
        mask; areas (m) i32 = set pixels): psalm_mask_boxes.  index (m) i32 on the device: the planes to describe (an entry outside [0, n) gives the
        empty result), default all n in order.  The outputs may be given (views of a caller-owned block); workspace: a caller's uint8 buffer of
        psalm_mask_boxes_workspace(m) bytes instead of the binding's cached one."""
        if masks.dim() != 3 or masks.dtype not in (torch.float32, torch.uint8, torch.bool):
            raise PsalmHipError(f"mask_boxes: masks (n,H,W) float32 / uint8 / bool, got {masks.dtype} {tuple(masks.shape)}")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        n, Hh, Ww = masks.shape
        m = n if index is None else int(index.numel())
        if index is not None:
            self._want(index, torch.int32, (m,), "mask_boxes index")
        boxes = self.empty(m, 4) if out_boxes is None else self._want(out_boxes, torch.float32, (m, 4), "mask_boxes out_boxes")
        areas = self.empty(m, dtype=torch.int32) if out_areas is None else self._want(out_areas, torch.int32, (m,), "mask_boxes out_areas")
        self.lib.psalm_mask_boxes_workspace.restype = c_long
        nbytes = self.lib.psalm_mask_boxes_workspace(m)
        if nbytes < 0:
            raise PsalmHipError(f"mask_boxes: {m} output rows (at most 65535)")
        if workspace is None:
            ws, have = self._stage_ws("mask_boxes", max(nbytes, 4)), nbytes
        else:
            if workspace.dtype != torch.uint8:
                raise PsalmHipError("mask_boxes: workspace must be a uint8 buffer")
            ws, have = workspace, int(workspace.numel())
        rc = self.lib.psalm_mask_boxes(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, Hh, Ww, self._p(index), m, self._p(boxes),
                                       self._p(areas), self._p(ws), c_long(have), self._stream())
        self._check(rc, "psalm_mask_boxes")
        return boxes, areas

    def label_boxes(self, labels, n_ids, out=None):
        """labels (H,W) int32 | uint8 -> table (n_ids,5) i32 of [x0, y0, x1, y1, area] per label value in [0, n_ids) (zeros for an absent value;
        other values are ignored), 1 <= n_ids <= 256: psalm_label_boxes.  `out` may be given (a view of a caller-owned block)."""
        if labels.dim() != 2 or labels.dtype not in (torch.int32, torch.uint8):
            raise PsalmHipError(f"label_boxes: labels (H,W) int32 / uint8, got {labels.dtype} {tuple(labels.shape)}")
        n_ids = int(n_ids)
        if not 1 <= n_ids <= 256:
            raise PsalmHipError(f"label_boxes: n_ids = {n_ids} (1..256)")
        Hh, Ww = labels.shape
        table = self.empty(n_ids, 5, dtype=torch.int32) if out is None else self._want(out, torch.int32, (n_ids, 5), "label_boxes out")
        rc = self.lib.psalm_label_boxes(self._p(labels), 1 if labels.dtype == torch.uint8 else 0, Hh, Ww, n_ids, self._p(table), self._stream())
        self._check(rc, "psalm_label_boxes")
        return table

    # ------------------------------------------------------------------ all-pairs mask overlap on bit planes (csrc/maskpairs.hip)
    MASK_PAIRS_MAX = 1024

    def mask_bits_words(self, HW) -> int:
        """words per bit plane of HW pixels, ceil(HW / 64): psalm_mask_bits_words"""
        fn = self._cdll_raw.psalm_mask_bits_words                      # (a host function: no launch to record)
        fn.restype = c_long
        nw = fn(c_long(int(HW)))
        if nw < 0:
            raise PsalmHipError(f"mask bit planes: {HW} pixels per plane (1 .. 2^31 - 1)")
        return int(nw)

    def _want_bits(self, bits, what):
        if not torch.is_tensor(bits) or bits.dim() != 2 or bits.dtype != torch.int64 or not bits.is_contiguous():
            raise PsalmHipError(f"{what}: bit planes (m,nw) as a contiguous int64 tensor, got {getattr(bits, 'dtype', type(bits))} "
                                f"{tuple(getattr(bits, 'shape', ()))}")
        return bits

    def mask_pack_bits(self, masks, index=None, out_bits=None, out_areas=None, want_areas=True):
        """masks (n,H,W) | (n,HW) float32 (set: > 0) | uint8 / bool (set: != 0) -> (bits (m,nw) int64: word w, bit b = pixel 64 w + b, the last word's
        tail zero; areas (m) i32 = set pixels, None with want_areas=False): psalm_mask_pack_bits.  index (m) i32 on the device: the planes to pack
        (an entry outside [0, n) gives an empty plane), default all n in order.  The outputs may be given (views of a caller-owned block)."""
        if not torch.is_tensor(masks) or masks.dim() not in (2, 3) or masks.dtype not in (torch.float32, torch.uint8, torch.bool):
            raise PsalmHipError(f"mask_pack_bits: masks (n,H,W) float32 / uint8 / bool, got {getattr(masks, 'dtype', type(masks))} "
                                f"{tuple(getattr(masks, 'shape', ()))}")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        n = int(masks.shape[0])
        HW = int(masks[0].numel()) if n else int(np.prod(masks.shape[1:]))
        nw = self.mask_bits_words(HW)
        m = n if index is None else int(index.numel())
        if index is not None:
            self._want(index, torch.int32, (m,), "mask_pack_bits index")
        if m > 65535:
            raise PsalmHipError(f"mask_pack_bits: {m} output rows (at most 65535)")
        bits = self.empty(m, nw, dtype=torch.int64) if out_bits is None else self._want(out_bits, torch.int64, (m, nw), "mask_pack_bits out_bits")
        areas = None
        if want_areas or out_areas is not None:
            areas = self.empty(m, dtype=torch.int32) if out_areas is None else self._want(out_areas, torch.int32, (m,), "mask_pack_bits out_areas")
        rc = self.lib.psalm_mask_pack_bits(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, c_long(HW), self._p(index), m, self._p(bits),
                                           self._p(areas), self._stream())
        self._check(rc, "psalm_mask_pack_bits")
        return bits, areas

    def mask_unpack_bits(self, bits, shape, rows=None, out=None):
        """bits (m,nw) int64, shape = (H, W) (or the pixel count HW) -> (k,H,W) | (k,HW) uint8 of 0 / 1 from the bit rows rows[i] ((k) i32 on the
        device, each below m; a negative entry gives an all-zero plane), default all m rows in order: psalm_mask_unpack_bits."""
        self._want_bits(bits, "mask_unpack_bits")
        dims = tuple(int(v) for v in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        HW = int(np.prod(dims))
        m, nw = bits.shape
        if self.mask_bits_words(HW) != nw:
            raise PsalmHipError(f"mask_unpack_bits: planes of {HW} pixels have {self.mask_bits_words(HW)} words, the bit rows have {nw}")
        k = m if rows is None else int(rows.numel())
        if rows is not None:
            self._want(rows, torch.int32, (k,), "mask_unpack_bits rows")
        if k > 65535:
            raise PsalmHipError(f"mask_unpack_bits: {k} output rows (at most 65535)")
        out = self.empty(k, *dims, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (k,) + dims, "mask_unpack_bits out")
        rc = self.lib.psalm_mask_unpack_bits(self._p(bits), c_long(nw), self._p(rows), k, c_long(HW), self._p(out), self._stream())
        self._check(rc, "psalm_mask_unpack_bits")
        return out

    def mask_pair_counts(self, bits_a, bits_b=None, out=None):
        """bits_a (ma,nw), bits_b (mb,nw) int64 bit planes (default: a against itself) -> inter (ma,mb) i32 = popcount(a_i & b_j) over the words,
        1 <= ma, mb <= 1024: psalm_mask_pair_counts.  `out` may be given; the call zeroes it itself."""
        self._want_bits(bits_a, "mask_pair_counts")
        bits_b = bits_a if bits_b is None else self._want_bits(bits_b, "mask_pair_counts")
        (ma, nw), (mb, nwb) = bits_a.shape, bits_b.shape
        if nw != nwb or nw < 1:
            raise PsalmHipError(f"mask_pair_counts: bit rows of {nw} and {nwb} words")
        if not (1 <= ma <= self.MASK_PAIRS_MAX and 1 <= mb <= self.MASK_PAIRS_MAX):
            raise PsalmHipError(f"mask_pair_counts: {ma} x {mb} planes (1..{self.MASK_PAIRS_MAX} per side)")
        inter = self.empty(ma, mb, dtype=torch.int32) if out is None else self._want(out, torch.int32, (ma, mb), "mask_pair_counts out")
        rc = self.lib.psalm_mask_pair_counts(self._p(bits_a), ma, self._p(bits_b), mb, c_long(nw), self._p(inter), self._stream())
        self._check(rc, "psalm_mask_pair_counts")
        return inter

    def mask_nms(self, inter, areas, scores, thr_num, thr_den, min_area=1, min_score=None, out_kept=None, out_keep=None, out_owner=None):
        """Greedy NMS on inter (m,m) i32, areas (m) i32, scores (m) f32 (NaN-free), 1 <= m <= 1024, under IoU > thr_num / thr_den (exact, strict;
        0 < thr_num <= thr_den <= 4096): psalm_mask_nms.  Descending score, equal scores the lowest index first; min_area / min_score filter
        (min_score=None: no score filter).  -> (kept (m + 1) i32 = [K, the K kept indices in rank order, -1 ...], keep (m) i32 = 1 kept / 0
        suppressed / -1 filtered, owner (m) i32 = the kept candidate standing for each, -1 if filtered)."""
        if not torch.is_tensor(inter) or inter.dim() != 2 or inter.shape[0] != inter.shape[1]:
            raise PsalmHipError(f"mask_nms: inter (m,m) int32, got {tuple(getattr(inter, 'shape', ()))}")
        m = int(inter.shape[0])
        if not 1 <= m <= self.MASK_PAIRS_MAX:
            raise PsalmHipError(f"mask_nms: {m} candidates (1..{self.MASK_PAIRS_MAX})")
        self._want(inter, torch.int32, (m, m), "mask_nms inter")
        self._want(areas, torch.int32, (m,), "mask_nms areas")
        self._want(scores, torch.float32, (m,), "mask_nms scores")
        thr_num, thr_den = int(thr_num), int(thr_den)
        if not (0 < thr_num <= thr_den <= 4096):
            raise PsalmHipError(f"mask_nms: threshold {thr_num}/{thr_den} (0 < thr_num <= thr_den <= 4096)")
        kept = self.empty(m + 1, dtype=torch.int32) if out_kept is None else self._want(out_kept, torch.int32, (m + 1,), "mask_nms out_kept")
        keep = self.empty(m, dtype=torch.int32) if out_keep is None else self._want(out_keep, torch.int32, (m,), "mask_nms out_keep")
        owner = self.empty(m, dtype=torch.int32) if out_owner is None else self._want(out_owner, torch.int32, (m,), "mask_nms out_owner")
        ms = float("-inf") if min_score is None else float(min_score)
        rc = self.lib.psalm_mask_nms(self._p(inter), self._p(areas), self._p(scores), m, thr_num, thr_den, int(min_area), c_float(ms), self._p(kept),
                                     self._p(keep), self._p(owner), self._stream())
        self._check(rc, "psalm_mask_nms")
        return kept, keep, owner

    def mask_paint_bits(self, bits, kept, shape, out=None):
        """bits (m,nw) int64, kept (m + 1) i32 as psalm_mask_nms writes it (K read on the device), shape = (H, W) (or HW) -> labels (H,W) i32:
        1 + the first k < K whose bit row kept[1 + k] holds the pixel, 0 for none: psalm_mask_paint_bits."""
        self._want_bits(bits, "mask_paint_bits")
        dims = tuple(int(v) for v in shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        HW = int(np.prod(dims))
        m, nw = bits.shape
        if self.mask_bits_words(HW) != nw:
            raise PsalmHipError(f"mask_paint_bits: planes of {HW} pixels have {self.mask_bits_words(HW)} words, the bit rows have {nw}")
        if not 1 <= m <= self.MASK_PAIRS_MAX:
            raise PsalmHipError(f"mask_paint_bits: {m} bit rows (1..{self.MASK_PAIRS_MAX})")
        self._want(kept, torch.int32, (m + 1,), "mask_paint_bits kept")
        labels = self.empty(*dims, dtype=torch.int32) if out is None else self._want(out, torch.int32, dims, "mask_paint_bits out")
        rc = self.lib.psalm_mask_paint_bits(self._p(bits), c_long(nw), self._p(kept), m, c_long(HW), self._p(labels), self._stream())
        self._check(rc, "psalm_mask_paint_bits")
        return labels

    # ------------------------------------------------------------------ connected components of binary planes (csrc/components.hip)
    COMPONENTS_WS_BYTES = 256 << 20

    def _planes_args(self, masks, index, connectivity, what):
        if not torch.is_tensor(masks) or masks.dim() != 3 or masks.dtype not in (torch.float32, torch.uint8, torch.bool):
            raise PsalmHipError(f"{what}: masks (n,H,W) float32 / uint8 / bool, got {getattr(masks, 'dtype', type(masks))} "
                                f"{tuple(getattr(masks, 'shape', ()))}")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        if connectivity not in (4, 8) or isinstance(connectivity, bool):
            raise PsalmHipError(f"{what}: connectivity {connectivity!r} (4 or 8)")
        n, Hh, Ww = (int(v) for v in masks.shape)
        if Hh * Ww >= 1 << 31:
            raise PsalmHipError(f"{what}: planes of {Hh} x {Ww} pixels (H * W < 2^31)")
        m = n if index is None else int(index.numel())
        if index is not None:
            self._want(index, torch.int32, (m,), f"{what} index")
        if m > 65535:
            raise PsalmHipError(f"{what}: {m} output rows (at most 65535)")
        return masks, n, Hh, Ww, m

    def _plane_chunks(self, fn, m, Hh, Ww, max_workspace_bytes, what):
        """[(first row, rows, workspace bytes)]: the m output rows in chunks whose workspace stays under max_workspace_bytes (at least one row)"""
        max_ws = self.COMPONENTS_WS_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
        if max_ws < 0:
            raise PsalmHipError(f"{what}: max_workspace_bytes = {max_ws}")
        fn.restype = c_long
        one = int(fn(1, Hh, Ww))
        if one < 0:
            raise PsalmHipError(f"{what}: planes of {Hh} x {Ww} pixels (H * W < 2^31)")
        per = max(1, min(m, max_ws // one if one else m))
        return [(r0, min(per, m - r0), int(fn(min(per, m - r0), Hh, Ww))) for r0 in range(0, m, per)]

    def mask_components(self, masks, index=None, connectivity=8, invert=False, max_components=256, want_table=True, max_workspace_bytes=None):
        """masks (n,H,W) float32 (set: > 0) | uint8 / bool (set: != 0) -> (labels (m,H,W) i32: 1 + the rank of the pixel's component among the plane's
        components ordered by their lowest row-major pixel, 0 for the other class; count (m) i32; table (m,max_components,6) i32 of [x0, y0, x1, y1,
        area, border] per component, None with want_table=False): psalm_mask_components.  index (m) i32 on the device: the planes to label (an entry
        outside [0, n) is the empty plane), default all n in order; invert: label the unset pixels.  The rows are walked in chunks whose workspace
        (three int32 planes per row) stays under max_workspace_bytes (default 256 MiB; at least one row per chunk): the result does not depend on it."""
        masks, n, Hh, Ww, m = self._planes_args(masks, index, connectivity, "mask_components")
        max_comp = int(max_components)
        if want_table and not 1 <= max_comp <= 65536:
            raise PsalmHipError(f"mask_components: max_components = {max_components} (1..65536)")
        labels = self.empty(m, Hh, Ww, dtype=torch.int32)
        count = self.empty(m, dtype=torch.int32)
        table = self.empty(m, max_comp, 6, dtype=torch.int32) if want_table else None
        if m == 0:
            return labels, count, table
        chunks = self._plane_chunks(self.lib.psalm_mask_components_workspace, m, Hh, Ww, max_workspace_bytes, "mask_components")
        if index is None and len(chunks) > 1:
            index = self._iota(n)                                     # a chunk of rows is a piece of the index list
        for r0, k, nbytes in chunks:
            ws = self._stage_ws("mask_components", max(nbytes, 4))
            rc = self.lib.psalm_mask_components(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, Hh, Ww,
                                                self._p(index[r0:r0 + k]) if index is not None else c_void_p(0), k,
                                                int(connectivity), 1 if invert else 0, self._p(labels[r0:r0 + k]), self._p(count[r0:r0 + k]),
                                                self._p(table[r0:r0 + k]) if want_table else c_void_p(0), max_comp if want_table else 1,
                                                self._p(ws), c_long(nbytes), self._stream())
            self._check(rc, "psalm_mask_components")
        return labels, count, table

    def mask_clean(self, masks, index=None, connectivity=8, min_island=0, max_hole=0, out=None, out_areas=None, out_filled=None, out_removed=None,
                   max_workspace_bytes=None):
        """masks (n,H,W) float32 (set: > 0) | uint8 / bool (set: != 0) -> (out (m,H,W) u8 of 0 / 1, areas (m) i32 of the cleaned planes, filled (m)
        i32, removed (m) i32): psalm_mask_clean.  First the holes -- components of the unset pixels under the complementary connectivity that miss
        the image border -- of at most max_hole pixels become set, then the islands of fewer than min_island pixels are cleared; a parameter of 0
        skips its step.  index (m) i32 on the device as in mask_components; the outputs may be given (views of a caller-owned block); chunked as
        mask_components."""
        masks, n, Hh, Ww, m = self._planes_args(masks, index, connectivity, "mask_clean")
        min_island, max_hole = int(min_island), int(max_hole)
        if min_island < 0 or max_hole < 0:
            raise PsalmHipError(f"mask_clean: min_island = {min_island}, max_hole = {max_hole} (both >= 0)")
        out = self.empty(m, Hh, Ww, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (m, Hh, Ww), "mask_clean out")
        areas = self.empty(m, dtype=torch.int32) if out_areas is None else self._want(out_areas, torch.int32, (m,), "mask_clean out_areas")
        filled = self.empty(m, dtype=torch.int32) if out_filled is None else self._want(out_filled, torch.int32, (m,), "mask_clean out_filled")
        removed = self.empty(m, dtype=torch.int32) if out_removed is None else self._want(out_removed, torch.int32, (m,), "mask_clean out_removed")
        if m == 0:
            return out, areas, filled, removed
        labelling = min_island > 0 or max_hole > 0
        chunks = self._plane_chunks(self.lib.psalm_mask_clean_workspace, m, Hh, Ww, max_workspace_bytes, "mask_clean") if labelling else [(0, m, 0)]
        if index is None and len(chunks) > 1:
            index = self._iota(n)
        for r0, k, nbytes in chunks:
            ws = self._stage_ws("mask_components", max(nbytes, 4)) if labelling else None
            rc = self.lib.psalm_mask_clean(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, Hh, Ww,
                                           self._p(index[r0:r0 + k]) if index is not None else c_void_p(0), k, int(connectivity), min_island, max_hole,
                                           self._p(out[r0:r0 + k]), self._p(areas[r0:r0 + k]), self._p(filled[r0:r0 + k]), self._p(removed[r0:r0 + k]),
                                           self._p(ws), c_long(nbytes), self._stream())
            self._check(rc, "psalm_mask_clean")
        return out, areas, filled, removed

    # ------------------------------------------------------------------ mask outlines and polygon fill (csrc/outlines.hip)
    def mask_outlines(self, masks, index=None, connectivity=8, max_workspace_bytes=None):
        """masks (n,H,W) float32 (set: > 0) | uint8 / bool (set: != 0) -> (ring_count (m) i32, vertex_count (m) i32, rings (R,4) i32 = [output row,
        first vertex offset, vertex count, signed area], vertices (V,2) i32 = (x, y)): psalm_mask_outline_totals + psalm_mask_outlines.  The crack
        edges between set and unset pixels, directed with the set pixel on the right, joined at saddles by `connectivity`, as closed rings of
        corner vertices; every ring starts at its row-major lowest vertex, a plane's rings are ordered by it; area > 0: an outer boundary, < 0: a
        hole.  index (m) i32 on the device: the planes to outline (an entry outside [0, n) is the empty plane), default all n in order.
        (H + 1) * (W + 1) * 4 < 2^31.  Two read-backs of small per-plane integers: the edge and corner totals that size the tables and the work,
        and the ring counts that trim the ring table.  The rows are walked in chunks whose workspace (proportional to the planes' edges, plus five
        bytes per lattice vertex) stays under max_workspace_bytes (default 256 MiB; at least one row per chunk): the result does not depend on it."""
        masks, n, Hh, Ww, m = self._planes_args(masks, index, connectivity, "mask_outlines")
        if (Hh + 1) * (Ww + 1) * 4 >= 1 << 31:
            raise PsalmHipError(f"mask_outlines: planes of {Hh} x {Ww} pixels ((H + 1) * (W + 1) * 4 < 2^31)")
        counts = self.empty(3, m, dtype=torch.int32)                  # [edges | vertices | rings] per output row
        if m == 0:
            return counts[2], counts[1], self.empty(0, 4, dtype=torch.int32), self.empty(0, 2, dtype=torch.int32)
        u8 = 1 if masks.dtype == torch.uint8 else 0
        rc = self.lib.psalm_mask_outline_totals(self._p(masks), u8, n, Hh, Ww, self._p(index), m, self._p(counts), self._stream())
        self._check(rc, "psalm_mask_outline_totals")
        edges, verts = counts[:2].cpu().numpy().astype(np.int64)      # read-back 1: 2 m small integers size everything below
        V, cap = int(verts.sum()), int(edges.max())
        if V >= 1 << 31:
            raise PsalmHipError(f"mask_outlines: {V} vertices in one call (< 2^31): outline fewer planes at a time")
        ring_cap = V // 4                                             # a ring has at least four corners
        rings = self.empty(ring_cap, 4, dtype=torch.int32)
        vertices = self.empty(V, 2, dtype=torch.int32)
        if cap == 0:
            return counts[2], counts[1], rings, vertices
        ws_fn = self.lib.psalm_mask_outlines_workspace
        ws_fn.restype = c_long

        def per_rows(k, h, w):
            return ws_fn(k, h, w, cap)
        for r0, k, nbytes in self._plane_chunks(per_rows, m, Hh, Ww, max_workspace_bytes, "mask_outlines"):
            ws = self._stage_ws("mask_outlines", max(nbytes, 16))
            rc = self.lib.psalm_mask_outlines(self._p(masks), u8, n, Hh, Ww, self._p(index), m, r0, k, int(connectivity), int(edges[r0:r0 + k].max()),
                                              self._p(counts), self._p(rings), ring_cap, self._p(vertices), V, self._p(ws), c_long(nbytes),
                                              self._stream())
            self._check(rc, "psalm_mask_outlines")
        R = int(counts[2].cpu().numpy().astype(np.int64).sum())       # read-back 2: the ring counts trim the table
        return counts[2], counts[1], rings[:R], vertices

    def mask_fill_polygons(self, rings, vertices, shape, out=None, max_workspace_bytes=None, rows=None):
        """rings (R,4) i32 = [plane, first vertex offset, vertex count, anything], vertices (V,2) i32 = (x, y) on the device, shape = (m, H, W) -> (m,H,W)
        uint8 of 0 / 1: psalm_mask_fill_polygons, the even-odd fill over pixel centres.  The tables of mask_outlines give the planes back bit for bit;
        any integer polygons in that layout are filled by the same rule (holes are rings; a ring given twice cancels).  A ring whose plane is
        outside [0, m) or whose vertex range leaves the table is passed over.  `out` may be given (a view of a caller-owned block); chunked as
        mask_components (one int32 per pixel of workspace).  rows = (first, k): only the planes [first, first + k) of the m are filled, into an
        `out` of (k, H, W)."""
        if not torch.is_tensor(rings) or rings.dim() != 2 or rings.shape[1] != 4:
            raise PsalmHipError(f"mask_fill_polygons: rings (R,4) int32, got {tuple(getattr(rings, 'shape', ()))}")
        if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 2:
            raise PsalmHipError(f"mask_fill_polygons: vertices (V,2) int32, got {tuple(getattr(vertices, 'shape', ()))}")
        R, V = int(rings.shape[0]), int(vertices.shape[0])
        self._want(rings, torch.int32, (R, 4), "mask_fill_polygons rings")
        self._want(vertices, torch.int32, (V, 2), "mask_fill_polygons vertices")
        if not isinstance(shape, (tuple, list)) or len(shape) != 3 or any(isinstance(v, bool) or int(v) != v or int(v) < 0 for v in shape):
            raise PsalmHipError(f"mask_fill_polygons: shape {shape!r} (m, H, W)")
        m, Hh, Ww = (int(v) for v in shape)
        if m > 65535 or (Hh + 1) * (Ww + 1) * 4 >= 1 << 31:
            raise PsalmHipError(f"mask_fill_polygons: {m} planes of {Hh} x {Ww} pixels (at most 65535 planes, (H + 1) * (W + 1) * 4 < 2^31)")
        first, m_out = (0, m) if rows is None else (int(rows[0]), int(rows[1]))
        if not (0 <= first and 0 <= m_out and first + m_out <= m):
            raise PsalmHipError(f"mask_fill_polygons: rows {rows!r} outside the {m} planes")
        out = self.empty(m_out, Hh, Ww, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (m_out, Hh, Ww), "mask_fill_polygons out")
        if m_out == 0 or Hh == 0 or Ww == 0:
            return out
        for r0, k, nbytes in self._plane_chunks(self.lib.psalm_mask_fill_polygons_workspace, m_out, Hh, Ww, max_workspace_bytes, "mask_fill_polygons"):
            ws = self._stage_ws("mask_fill_polygons", max(nbytes, 4))
            rc = self.lib.psalm_mask_fill_polygons(self._p(rings), R, self._p(vertices), V, first + r0, k, Hh, Ww, self._p(out[r0:r0 + k]), self._p(ws),
                                                   c_long(nbytes), self._stream())
            self._check(rc, "psalm_mask_fill_polygons")
        return out

    # ------------------------------------------------------------------ mask distance maps (csrc/distance.hip)
    DISTANCE_MAX_SIDE = 16384
    DISTANCE_FAR = 1 << 30
    BOUNDARY_MAX_BOUND = 32767

    def _distance_args(self, masks, index, what):
        """masks (n,H,W) float32 / uint8 / bool, 1 <= H, W <= 16384, at most 65535 output rows -> (masks as the kernels read them, n, H, W, m)"""
        if not torch.is_tensor(masks) or masks.dim() != 3 or masks.dtype not in (torch.float32, torch.uint8, torch.bool):
            raise PsalmHipError(f"{what}: masks (n,H,W) float32 / uint8 / bool, got {getattr(masks, 'dtype', type(masks))} "
                                f"{tuple(getattr(masks, 'shape', ()))}")
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        n, Hh, Ww = (int(v) for v in masks.shape)
        if not (1 <= Hh <= self.DISTANCE_MAX_SIDE and 1 <= Ww <= self.DISTANCE_MAX_SIDE):
            raise PsalmHipError(f"{what}: planes of {Hh} x {Ww} pixels (1 <= H, W <= {self.DISTANCE_MAX_SIDE})")
        m = n if index is None else int(index.numel())
        if index is not None:
            self._want(index, torch.int32, (m,), f"{what} index")
        if m > 65535:
            raise PsalmHipError(f"{what}: {m} output rows (at most 65535)")
        return masks, n, Hh, Ww, m

    def _aligned_ws(self, name, nbytes):
        """_stage_ws, cut to start on a 256-byte boundary (the distance entries ask for it; the host allocator of the emulation gives 64)"""
        t = self._stage_ws(name, nbytes + 256)
        off = (-t.data_ptr()) % 256
        return t[off:off + nbytes]

    def mask_distance(self, masks, index=None, to="unset", border=False, out=None, max_workspace_bytes=None):
        """masks (n,H,W) float32 (set: > 0) | uint8 / bool (set: != 0) -> dist2 (m,H,W) i32, the exact squared Euclidean distance of every pixel to the
        nearest seed pixel: psalm_mask_distance.  to="unset": the seeds are the unset pixels (the inside distance, 0 off the mask); to="set": the set
        pixels.  border=True: every position outside the image is a seed too.  DISTANCE_FAR = 2^30 where there is no seed at all.  index (m) i32 on
        the device: the planes to transform (an entry outside [0, n) is the empty plane), default all n in order.  1 <= H, W <= 16384.  `out` may
        be given; the rows are walked in chunks whose workspace (six bytes per pixel) stays under max_workspace_bytes (default 256 MiB; at least
        one row per chunk): the result does not depend on it."""
        masks, n, Hh, Ww, m = self._distance_args(masks, index, "mask_distance")
        if to not in ("unset", "set"):
            raise PsalmHipError(f"mask_distance: to = {to!r} ('unset': distance to the unset pixels, or 'set')")
        if not isinstance(border, (bool, np.bool_)):
            raise PsalmHipError(f"mask_distance: border = {border!r} (True or False)")
        out = self.empty(m, Hh, Ww, dtype=torch.int32) if out is None else self._want(out, torch.int32, (m, Hh, Ww), "mask_distance out")
        if m == 0:
            return out
        chunks = self._plane_chunks(self.lib.psalm_mask_distance_workspace, m, Hh, Ww, max_workspace_bytes, "mask_distance")
        if index is None and len(chunks) > 1:
            index = self._iota(n)
        for r0, k, nbytes in chunks:
            ws = self._aligned_ws("mask_distance", nbytes)
            rc = self.lib.psalm_mask_distance(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, Hh, Ww,
                                              self._p(index[r0:r0 + k]) if index is not None else c_void_p(0), k, 1 if to == "set" else 0,
                                              1 if border else 0, self._p(out[r0:r0 + k]), self._p(ws), c_long(nbytes), self._stream())
            self._check(rc, "psalm_mask_distance")
        return out

    def mask_centers(self, masks, index=None, dist2=None, out=None, max_workspace_bytes=None):
        """masks (n,H,W) float32 | uint8 / bool -> centers (m,3) i32 = [y, x, dist2] of each plane's set pixel deepest inside -- the first maximum, in
        row-major order, of mask_distance(to="unset", border=True) over the set pixels; [-1, -1, 0] for an empty plane: psalm_mask_centers.  dist2
        (m,H,W) i32: that map when the caller has it; otherwise it is made here, chunk by chunk (ten bytes per pixel under max_workspace_bytes,
        default 256 MiB), and dropped."""
        masks, n, Hh, Ww, m = self._distance_args(masks, index, "mask_centers")
        out = self.empty(m, 3, dtype=torch.int32) if out is None else self._want(out, torch.int32, (m, 3), "mask_centers out")
        if dist2 is not None:
            self._want(dist2, torch.int32, (m, Hh, Ww), "mask_centers dist2")
        if m == 0:
            return out
        u8 = 1 if masks.dtype == torch.uint8 else 0
        slots = self.empty(m, dtype=torch.int64)
        if dist2 is not None:
            chunks = [(0, m, 0)]
        else:
            ws_fn = self.lib.psalm_mask_distance_workspace
            ws_fn.restype = c_long
            chunks = self._plane_chunks(lambda k, h, w: ws_fn(k, h, w) + (k * h * w * 4 if ws_fn(k, h, w) >= 0 else 0), m, Hh, Ww, max_workspace_bytes,
                                        "mask_centers")
        if index is None and len(chunks) > 1:
            index = self._iota(n)
        for r0, k, nbytes in chunks:
            idx = self._p(index[r0:r0 + k]) if index is not None else c_void_p(0)
            if dist2 is None:
                wsb = int(ws_fn(k, Hh, Ww))
                blk = self._aligned_ws("mask_centers", nbytes)
                d = blk[wsb:wsb + k * Hh * Ww * 4].view(torch.int32).view(k, Hh, Ww)
                rc = self.lib.psalm_mask_distance(self._p(masks), u8, n, Hh, Ww, idx, k, 0, 1, self._p(d), self._p(blk), c_long(wsb), self._stream())
                self._check(rc, "psalm_mask_distance")
            else:
                d = dist2
            rc = self.lib.psalm_mask_centers(self._p(masks), u8, n, Hh, Ww, idx, k, self._p(d), self._p(slots[r0:r0 + k]), self._p(out[r0:r0 + k]),
                                             self._stream())
            self._check(rc, "psalm_mask_centers")
        return out

    def mask_boundaries(self, masks, index=None, out=None):
        """masks (n,H,W) float32 | uint8 / bool -> (m,H,W) uint8 of 0 / 1: DAVIS's seg2bmap at the mask's own size (a pixel that differs from its right,
        lower or lower-right neighbour; the last row looks right, the last column down, the last pixel is 0): psalm_mask_boundaries."""
        masks, n, Hh, Ww, m = self._distance_args(masks, index, "mask_boundaries")
        out = self.empty(m, Hh, Ww, dtype=torch.uint8) if out is None else self._want(out, torch.uint8, (m, Hh, Ww), "mask_boundaries out")
        if m:
            rc = self.lib.psalm_mask_boundaries(self._p(masks), 1 if masks.dtype == torch.uint8 else 0, n, Hh, Ww, self._p(index), m, self._p(out),
                                                self._stream())
            self._check(rc, "psalm_mask_boundaries")
        return out

    def boundary_counts(self, pred, gt, pair_pred, pair_gt, bound, pred_index=None, gt_index=None):
        """pred (n,H,W), gt (k,H,W) float32 | uint8 / bool, pair_pred / pair_gt (P) i32 on the device -> counts (P,4) i64 = [n_fg, n_gt, fg_match,
        gt_match] of DAVIS's boundary F per pair: psalm_boundary_counts.  pred_index / gt_index (i32 on the device): the planes that take part
        (the pairs then index into these lists), default all.  0 <= bound <= 32767: a boundary pixel matches when the other boundary has a pixel
        within dy^2 + dx^2 <= bound^2.  Boundary and near maps are made once per plane; the workspace holds two bytes per pixel of them."""
        pred, n_p, Hh, Ww, mp = self._distance_args(pred, pred_index, "boundary_counts")
        gt, n_t, Ht, Wt, mt = self._distance_args(gt, gt_index, "boundary_counts")
        if (Hh, Ww) != (Ht, Wt):
            raise PsalmHipError(f"boundary_counts: predictions of {Hh} x {Ww} against targets of {Ht} x {Wt}")
        if isinstance(bound, (bool, np.bool_)) or not isinstance(bound, (int, np.integer)) or not 0 <= int(bound) <= self.BOUNDARY_MAX_BOUND:
            raise PsalmHipError(f"boundary_counts: bound = {bound!r} (an integer, 0 <= bound <= {self.BOUNDARY_MAX_BOUND})")
        if not torch.is_tensor(pair_pred) or not torch.is_tensor(pair_gt) or pair_pred.dim() != 1 or pair_pred.shape != pair_gt.shape:
            raise PsalmHipError("boundary_counts: pair_pred / pair_gt (P) int32 of one length")
        P = int(pair_pred.numel())
        self._want(pair_pred, torch.int32, (P,), "boundary_counts pair_pred")
        self._want(pair_gt, torch.int32, (P,), "boundary_counts pair_gt")
        if P > 65535 or mp + mt > 65535:
            raise PsalmHipError(f"boundary_counts: {P} pairs over {mp} + {mt} planes (at most 65535 pairs, 65535 planes)")
        counts = self.empty(P, 4, dtype=torch.int64)
        if P == 0:
            return counts
        ws_fn = self.lib.psalm_boundary_counts_workspace
        ws_fn.restype = c_long
        nbytes = int(ws_fn(mp, mt, Hh, Ww))
        ws = self._aligned_ws("boundary_counts", nbytes)
        rc = self.lib.psalm_boundary_counts(self._p(pred), 1 if pred.dtype == torch.uint8 else 0, n_p, self._p(pred_index), mp,
                                            self._p(gt), 1 if gt.dtype == torch.uint8 else 0, n_t, self._p(gt_index), mt, Hh, Ww,
                                            self._p(pair_pred), self._p(pair_gt), P, int(bound), self._p(counts), self._p(ws), c_long(nbytes), self._stream())
        self._check(rc, "psalm_boundary_counts")
        return counts

    # ------------------------------------------------------------------ panoptic quality (csrc/panopticq.hip)
    LABEL_PAIRS_MAX_IDS = 1023
    PQ_MAX_CATEGORIES = 4096

    def _id_map(self, t, what):
        """an id map as the kernels read it: (H,W) int32, or (H,W,3) uint8 = the panoptic PNG's rgb -> (tensor, is_rgb, H, W)"""
        if not torch.is_tensor(t) or not ((t.dim() == 2 and t.dtype == torch.int32) or (t.dim() == 3 and t.shape[2] == 3 and t.dtype == torch.uint8)):
            raise PsalmHipError(f"{what}: an (H,W) int32 id map or its (H,W,3) uint8 rgb form, got {getattr(t, 'dtype', type(t))} "
                                f"{tuple(getattr(t, 'shape', ()))}")
        if not t.is_contiguous():
            raise PsalmHipError(f"{what}: the map must be contiguous")
        return t, 1 if t.dim() == 3 else 0, int(t.shape[0]), int(t.shape[1])

    def _id_table(self, ids, check, what):
        if not torch.is_tensor(ids) or ids.dim() != 1 or ids.dtype != torch.int32 or not ids.is_contiguous():
            raise PsalmHipError(f"{what}: a contiguous (n) int32 tensor, got {getattr(ids, 'dtype', type(ids))} {tuple(getattr(ids, 'shape', ()))}")
        n = int(ids.numel())
        if n > self.LABEL_PAIRS_MAX_IDS:
            raise PsalmHipError(f"{what}: {n} ids (at most {self.LABEL_PAIRS_MAX_IDS})")
        if check and n:
            v = ids.cpu().numpy().astype(np.int64)
            if v[0] <= 0 or (np.diff(v) <= 0).any():
                raise PsalmHipError(f"{what}: ids must be > 0 and strictly ascending")
        return n

    def label_pair_counts(self, gt, gt_ids, pred, pred_ids, out=None, check=True):
        """gt, pred: id maps of one size, each (H,W) int32 or (H,W,3) uint8 (id = R + 256 G + 65536 B); gt_ids (G), pred_ids (P): int32 on the device,
        strictly ascending, > 0, at most 1023 each -> counts (G+2, P+2) i32, overwritten: counts[a][b] = pixels whose gt value has slot a and whose
        pred value has slot b (slot 0: the value 0 = VOID; 1 + k: table entry k; last: any other value): psalm_label_pair_counts.  check=True reads
        the two tables back to verify their order (a caller that sorted them on the host passes False: the kernel's binary search relies on it).
        `out` may be given (a view of a caller-owned block)."""
        gt, g_rgb, Hh, Ww = self._id_map(gt, "label_pair_counts gt")
        pred, p_rgb, Hp, Wp = self._id_map(pred, "label_pair_counts pred")
        if (Hh, Ww) != (Hp, Wp):
            raise PsalmHipError(f"label_pair_counts: a ground truth of {Hh} x {Ww} against a prediction of {Hp} x {Wp}")
        if not 1 <= Hh * Ww <= 2 ** 31 - 1:
            raise PsalmHipError(f"label_pair_counts: {Hh} x {Ww} pixels (1 <= H * W <= 2^31 - 1)")
        G = self._id_table(gt_ids, check, "label_pair_counts gt_ids")
        P = self._id_table(pred_ids, check, "label_pair_counts pred_ids")
        counts = self.empty(G + 2, P + 2, dtype=torch.int32) if out is None else self._want(out, torch.int32, (G + 2, P + 2), "label_pair_counts out")
        rc = self.lib.psalm_label_pair_counts(self._p(gt), g_rgb, self._p(gt_ids), G, self._p(pred), p_rgb, self._p(pred_ids), P, Hh, Ww,
                                              self._p(counts), self._stream())
        self._check(rc, "psalm_label_pair_counts")
        return counts

    def pq_accumulate(self, counts, gt_cat, gt_crowd, pred_cat, pred_crowd_slot, stat, iou, notes):
        """counts (G+2, P+2) i32 of `label_pair_counts`; gt_cat, gt_crowd (G), pred_cat, pred_crowd_slot (P) i32 on the device (category slots in
        [0, C), crowd flags 0 / 1, per prediction the gt slot 1..G of its category's crowd segment or -1); the accumulators stat (C,3) i64 = [tp, fp,
        fn], iou (C) f64, notes (4) i64 are added to in place: psalm_pq_accumulate (panopticapi's pq_compute_single_core for one image; the IoU
        sums are added in its own order by one thread, so they are reproducible bit for bit).  Returns None."""
        if not torch.is_tensor(counts) or counts.dim() != 2 or counts.shape[0] < 2 or counts.shape[1] < 2:
            raise PsalmHipError(f"pq_accumulate: counts (G+2, P+2) int32, got {tuple(getattr(counts, 'shape', ()))}")
        G, P = int(counts.shape[0]) - 2, int(counts.shape[1]) - 2
        if G > self.LABEL_PAIRS_MAX_IDS or P > self.LABEL_PAIRS_MAX_IDS:
            raise PsalmHipError(f"pq_accumulate: {G} x {P} listed segments (at most {self.LABEL_PAIRS_MAX_IDS} per side)")
        self._want(counts, torch.int32, (G + 2, P + 2), "pq_accumulate counts")
        for t, n, what in ((gt_cat, G, "gt_cat"), (gt_crowd, G, "gt_crowd"), (pred_cat, P, "pred_cat"), (pred_crowd_slot, P, "pred_crowd_slot")):
            if not torch.is_tensor(t):
                raise PsalmHipError(f"pq_accumulate {what}: an int32 tensor on the device")
            self._want(t, torch.int32, (n,), "pq_accumulate " + what)
        if not torch.is_tensor(stat) or stat.dim() != 2:
            raise PsalmHipError("pq_accumulate: stat (C,3) int64")
        C = int(stat.shape[0])
        if not 1 <= C <= self.PQ_MAX_CATEGORIES:
            raise PsalmHipError(f"pq_accumulate: {C} categories (1..{self.PQ_MAX_CATEGORIES})")
        self._want(stat, torch.int64, (C, 3), "pq_accumulate stat")
        self._want(iou, torch.float64, (C,), "pq_accumulate iou")
        self._want(notes, torch.int64, (4,), "pq_accumulate notes")
        rc = self.lib.psalm_pq_accumulate(self._p(counts), G, P, self._p(gt_cat), self._p(gt_crowd), self._p(pred_cat), self._p(pred_crowd_slot), C,
                                          self._p(stat), self._p(iou), self._p(notes), self._stream())
        self._check(rc, "psalm_pq_accumulate")

    def _iota(self, n):
        """0 .. n - 1 as int32 on the device (cached per length)"""
        key = ("iota", n)
        t = self._ws.get(key)
        if t is None:
            t = self._ws[key] = torch.arange(n, dtype=torch.int32).to(self.device)
        return t


_OPS: Optional[Ops] = None


def get_ops() -> Ops:
    """The product accessor: libpsalm_hip.so on a GPU, or an exception."""
    global _OPS
    if _OPS is None:
        if not torch.cuda.is_available():
            raise PsalmHipError("no GPU visible: psalm_amd runs only on its HIP kernels (MI355X/gfx950); "
                                "there is deliberately no CPU fallback")
        _OPS = Ops(DEFAULT_LIB)
    return _OPS
