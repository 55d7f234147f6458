"""ctypes binding of ``libdsphere_hip.so`` (the C ABI declared in ``include/dsphere.h``).

There is no CPU fallback: if the shared library is missing, or a forward is requested
without a HIP device, this module raises.  Build the library with
``make -C deepsphere-cosmo-tf2_amd/csrc`` (or ``__graft_entry__.build()``).
"""

import ctypes
import os

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libdsphere_hip.so")
_lib = None

OK = 0
ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4
PREC_FP32, PREC_BF16X3, PREC_BF16X6, PREC_F16X3 = 0, 1, 2, 3
ALGO_AUTO, ALGO_UNFUSED, ALGO_FUSED = 0, 1, 2
PART_ALL, PART_INTERIOR, PART_BOUNDARY = 0, 1, 2
FWD_KEEP_WEIGHTS = 1
ABI_VERSION = 3  # DSPH_ABI_VERSION of include/dsphere.h this binding was written against
POOL_MAX, POOL_AVG = 0, 1
PREPARE_BACKWARD, PREPARE_RELEASE_HOST = 1, 2
BASIS_CHEBYSHEV, BASIS_MONOMIAL = 0, 1
# dsph_plan_set_option (include/dsphere.h: DSPH_OPT_*)
OPT_STRIPS, OPT_STRUCT, OPT_TABLES, OPT_FORK, OPT_STRIP_MINROWS, OPT_SPLIT, OPT_TSTEP = 1, 2, 3, 4, 6, 8, 9  # (5 and 7: retired, never reused)
OPT_PACK = 10
OPT_STRIP_FORM = 11
OPT_F16_XEXP = 12
OPT_QSTRIP_IMAGE = 13  # the K = 5 quad strips' packed image of L~: 0 automatic (on), 1 on, 2 off
STRIP_FORM_QUAD, STRIP_FORM_PAIRS = 0, 1
STRIPS_AUTO, STRIPS_ALWAYS, STRIPS_NEVER = 0, 1, 2
SPLIT_AUTO, SPLIT_ALWAYS, SPLIT_NEVER = 0, 1, 2

_c_i64 = ctypes.c_int64
_c_i32 = ctypes.c_int32
_c_vp = ctypes.c_void_p

# name -> (restype, argtypes); one entry per function declared in include/dsphere.h
SIGNATURES = {
    "dsph_abi_version": (ctypes.c_int, []),
    "dsph_last_error": (ctypes.c_char_p, []),
    "dsph_plan_create": (ctypes.c_int, [ctypes.POINTER(_c_vp), _c_i64, _c_i64, _c_i32, _c_vp, _c_vp, ctypes.c_int]),
    "dsph_plan_destroy": (None, [_c_vp]),
    "dsph_plan_set_levels": (ctypes.c_int, [_c_vp, _c_i32, _c_vp]),
    "dsph_plan_set_option": (ctypes.c_int, [_c_vp, _c_i32, _c_i64]),
    "dsph_plan_strip_pairs": (ctypes.c_int, [_c_vp, _c_i32, _c_vp, _c_i64, ctypes.POINTER(_c_i64)]),
    "dsph_plan_strip_split": (ctypes.c_int, [_c_vp, _c_i64, ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i32),
                                             ctypes.POINTER(_c_i64)]),
    "dsph_plan_strip_rows": (ctypes.c_int, [_c_vp, _c_i32, _c_i64, _c_i64, _c_vp, _c_vp]),
    "dsph_plan_strip_image": (ctypes.c_int, [_c_vp, _c_i32, _c_i64, _c_vp, _c_i64, ctypes.POINTER(_c_i64)]),
    "dsph_plan_rows": (_c_i64, [_c_vp]),
    "dsph_plan_cols": (_c_i64, [_c_vp]),
    "dsph_plan_ell_width": (_c_i32, [_c_vp]),
    "dsph_plan_out_rows": (_c_i64, [_c_vp, _c_i32]),
    "dsph_plan_fused_ok": (ctypes.c_int, [_c_vp, _c_i32, _c_i32, _c_i32]),
    "dsph_plan_uses_chain": (ctypes.c_int, [_c_vp, _c_i32, _c_i32, _c_i32]),
    "dsph_plan_prepare": (ctypes.c_int, [_c_vp, _c_i32, _c_i32, _c_i32]),
    "dsph_plan_prepare_layer": (ctypes.c_int, [_c_vp, _c_i32, _c_i32, _c_i32, _c_i32]),
    "dsph_plan_tile_counts": (ctypes.c_int, [_c_vp, _c_i32, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "dsph_plan_strip_tiles": (ctypes.c_int, [_c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, ctypes.POINTER(_c_i64)]),
    "dsph_workspace_bytes": (ctypes.c_size_t, [_c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "dsph_cheb_forward": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp,
         ctypes.c_size_t, _c_vp],
    ),
    "dsph_poly_forward": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp,
         ctypes.c_size_t, _c_vp],
    ),
    "dsph_poly_forward_part": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32,
         _c_vp, ctypes.c_size_t, _c_vp],
    ),
    "dsph_poly_forward_ex": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32,
         _c_vp, ctypes.c_size_t, _c_vp],
    ),
    "dsph_cheb_step": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, ctypes.c_float, ctypes.c_float, _c_i64, _c_vp],
    ),
    "dsph_cheb_contract": (
        ctypes.c_int,
        [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, ctypes.c_int,
         _c_vp],
    ),
    "dsph_wgrad_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i32, _c_i32, _c_i32]),
    "dsph_cheb_planes": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp],
    ),
    "dsph_backward_weights_workspace_bytes": (ctypes.c_size_t, [_c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32]),
    "dsph_cheb_backward_weights": (
        ctypes.c_int,
        [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp, ctypes.c_size_t,
         _c_vp],
    ),
    "dsph_cheb_wgrad": (
        ctypes.c_int,
        [_c_vp, _c_i64, _c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_vp, ctypes.c_size_t, ctypes.c_int,
         _c_vp],
    ),
    "dsph_rows_pack": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_vp, _c_i64, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_rows_unpack": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_vp, _c_i64, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_plan_pool_fusable": (ctypes.c_int, [_c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32]),
    "dsph_poly_forward_pool": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32,
                                               _c_i32, _c_i32, _c_i32, _c_vp, ctypes.c_size_t, _c_vp]),
    "dsph_healpix_pool": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_healpix_pool_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_healpix_reorder": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_healpix_knn": (ctypes.c_int, [_c_i32, _c_i32, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_vp]),
    "dsph_healpix_disc_count": (ctypes.c_int, [_c_i32, ctypes.c_double, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_vp]),
    "dsph_healpix_gauss_table": (ctypes.c_int, [_c_i32, _c_i32, ctypes.c_double, ctypes.c_double, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp,
                                                 ctypes.c_int, _c_vp]),
    "dsph_healpix_rotate": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_vp, _c_i64, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "dsph_healpix_interp_table": (ctypes.c_int, [_c_i32, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_vp]),
    "dsph_sht_ring_analysis": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "dsph_sht_legendre_analysis": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_sht_legendre_synthesis": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_sht_ring_synthesis": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_vp, _c_vp, _c_i64, ctypes.c_int, _c_vp]),
    "dsph_residual_epilogue": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_float, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_nbr_attention_forward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i32, _c_i64, _c_i64, _c_i32, _c_i32,
                                                   ctypes.c_int, _c_vp]),
    "dsph_nbr_attention_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_i32, _c_vp, _c_i32, _c_vp,
                                                    _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_dense_attention_forward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32, ctypes.c_int,
                                                     _c_vp]),
    "dsph_dense_attention_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64,
                                                      _c_i64, _c_i64, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_dense_attention_forward_prec": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_i64, _c_i64, _c_i32, _c_i32,
                                                          _c_i32, ctypes.c_int, _c_vp]),
    "dsph_dense_attention_backward_prec": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                                           _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_dense_attention_forward_masked": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64,
                                                            _c_i64, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_dense_attention_backward_masked": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp,
                                                             _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32,
                                                             ctypes.c_int, _c_vp]),
    "dsph_ell_smooth": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_vp, _c_vp, _c_i64, _c_i32, _c_vp, _c_i32, _c_vp, _c_i32,
                                        ctypes.c_int, _c_vp]),
    "dsph_basis_change": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_bn_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "dsph_bn_stats": (ctypes.c_int, [_c_vp, _c_i64, _c_i32, ctypes.c_float, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_float, _c_vp,
                                      ctypes.c_size_t, ctypes.c_int, _c_vp]),
    "dsph_bn_apply": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i32, _c_vp, _c_vp, _c_vp, _c_vp, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_bn_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_vp,
                                         ctypes.c_size_t, ctypes.c_int, _c_vp]),
    "dsph_ln_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "dsph_ln_forward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, ctypes.c_float, _c_vp, _c_vp, ctypes.c_int, _c_vp]),
    "dsph_ln_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_float, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_vp, ctypes.c_size_t,
                                         ctypes.c_int, _c_vp]),
    "dsph_patch_gemm": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, ctypes.c_int, _c_vp]),
    "dsph_patch_backward_workspace_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "dsph_patch_epilogue_backward": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_i32, _c_i32, _c_vp, ctypes.c_size_t, ctypes.c_int,
                                                    _c_vp]),
}


def library_path():
    return _LIB_PATH


def lib():
    """The loaded library; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"HIP library not found at {_LIB_PATH}: build it with "
                "`make -C deepsphere-cosmo-tf2_amd/csrc` (there is no CPU fallback)"
            )
        handle = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.dsph_abi_version() != ABI_VERSION:
            raise RuntimeError("libdsphere_hip.so has an unexpected ABI version")
        _lib = handle
    return _lib


def last_error():
    msg = lib().dsph_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what):
    if rc == OK:
        return
    msg = f"{what} failed ({rc}): {last_error()}"
    if rc == -1:
        raise ValueError(msg)
    raise RuntimeError(msg)


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "the Chebyshev forward runs only on a HIP device (MI355X); no GPU is visible and there is no CPU fallback"
        )


class LaplacianPlan:
    """Owner of one ``dsph_plan``: the rescaled Laplacian, padded ELL, resident on one GPU."""

    def __init__(self, ell_cols, ell_vals, n_cols=None, device=0, levels=None, options=None):
        cols = np.ascontiguousarray(ell_cols, dtype=np.int32)
        vals = np.ascontiguousarray(ell_vals, dtype=np.float32)
        if cols.ndim != 2 or cols.shape != vals.shape:
            raise ValueError("ELL cols/vals must be 2-D arrays of equal shape [rows, width]")
        self.n_rows, self.width = int(cols.shape[0]), int(cols.shape[1])
        self.n_cols = int(n_cols) if n_cols is not None else self.n_rows
        self.device = int(device)
        self._h = _c_vp()
        require_gpu()
        rc = lib().dsph_plan_create(
            ctypes.byref(self._h), self.n_rows, self.n_cols, self.width, cols.ctypes.data, vals.ctypes.data,
            self.device,
        )
        check(rc, "dsph_plan_create")
        self.levels = None
        if levels is not None:
            self.set_levels(levels)
        for opt, value in (options or {}).items():
            self.set_option(opt, value)

    def set_option(self, option, value):
        """``dsph_plan_set_option``: a per-plan choice (OPT_*), to be made before the tables of a K are built."""
        check(lib().dsph_plan_set_option(self.handle, int(option), int(value)), "dsph_plan_set_option")

    def set_levels(self, levels):
        lv = np.ascontiguousarray(levels, dtype=np.int64)
        check(lib().dsph_plan_set_levels(self._h, int(lv.shape[0]), lv.ctypes.data), "dsph_plan_set_levels")
        self.levels = lv.copy()

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("plan already destroyed")
        return self._h

    @property
    def out_rows(self):
        return int(lib().dsph_plan_out_rows(self.handle, 1))

    def fused_ok(self, Fin, Fout, K):
        return bool(lib().dsph_plan_fused_ok(self.handle, int(Fin), int(Fout), int(K)))

    def uses_chain(self, Fin, Fout, K):
        """``dsph_plan_uses_chain``: does a forward of this shape run as the chain of <= 5-term passes (K > 5)."""
        return bool(lib().dsph_plan_uses_chain(self.handle, int(Fin), int(Fout), int(K)))

    def prepare(self, K, Fin, backward=False, release_host=False, Fout=None):
        """Build the fused kernels' tables for a K-term layer now (``dsph_plan_prepare_layer``; without ``Fout`` the width is
        taken as ``Fin``): afterwards a forward neither allocates nor synchronises, so it can be timed and captured into a graph."""
        flags = (PREPARE_BACKWARD if backward else 0) | (PREPARE_RELEASE_HOST if release_host else 0)
        check(lib().dsph_plan_prepare_layer(self.handle, int(K), int(Fin), int(Fin if Fout is None else Fout), flags),
              "dsph_plan_prepare_layer")

    def tile_counts(self, K):
        """(tiles run by the structured-tile kernel, tiles run by the BFS-tile kernel) of a K-term fused forward."""
        a, b = _c_i64(0), _c_i64(0)
        check(lib().dsph_plan_tile_counts(self.handle, int(K), ctypes.byref(a), ctypes.byref(b)), "dsph_plan_tile_counts")
        return int(a.value), int(b.value)

    def strip_tiles(self, Fin, Fout, K, precision=PREC_BF16X3, N=1):
        """How many of the structured tiles a fused forward of this shape, on a batch of N maps, hands to the strip kernel
        (``dsph_plan_strip_tiles``)."""
        n = _c_i64(0)
        check(lib().dsph_plan_strip_tiles(self.handle, int(N), int(Fin), int(Fout), int(K), int(precision), ctypes.byref(n)),
              "dsph_plan_strip_tiles")
        return int(n.value)

    def strip_pairs(self, K):
        """The strip kernel's work list for K terms (``dsph_plan_strip_pairs``): an int32 array [n_pairs, 12] of
        x0[2], w[2], xs[2], y0, y1, xlo, xhi, ylo, yhi in the virtual Z-order plane of the row index."""
        n = _c_i64(0)
        check(lib().dsph_plan_strip_pairs(self.handle, int(K), _c_vp(), 0, ctypes.byref(n)), "dsph_plan_strip_pairs")
        out = np.zeros((int(n.value), 12), dtype=np.int32)
        if n.value:
            check(lib().dsph_plan_strip_pairs(self.handle, int(K), out.ctypes.data, int(n.value), ctypes.byref(n)),
                  "dsph_plan_strip_pairs")
        return out

    def strip_rows(self, K, strip, xs, ys):
        """Row numbers of the pixels (xs[i], ys[i]) of the plane of strip record ``strip`` (``dsph_plan_strip_rows``): through the
        rectangle's table of tile bases for the quad strips, the Z-order plane of the row index for the strip pairs."""
        xy = np.ascontiguousarray(np.stack([np.asarray(xs), np.asarray(ys)], axis=1), dtype=np.int32)
        rows = np.zeros(xy.shape[0], dtype=np.int64)
        check(lib().dsph_plan_strip_rows(self.handle, int(K), int(strip), int(xy.shape[0]), xy.ctypes.data, rows.ctypes.data),
              "dsph_plan_strip_rows")
        return rows

    def strip_image(self, strip, basis=0):
        """The packed image of L~ of K = 5 quad-strip record ``strip`` (``dsph_plan_strip_image``): a float32 array
        [yhi - ylo + 8, 9, 16, 4] -- rows ylo - 1 .. yhi + 6, the diagonal and the eight directions, p, tile; ``basis`` 0: doubled
        (Chebyshev), 1: as it stands (monomial)."""
        n = _c_i64(0)
        check(lib().dsph_plan_strip_image(self.handle, int(basis), int(strip), _c_vp(), 0, ctypes.byref(n)), "dsph_plan_strip_image")
        out = np.zeros(int(n.value), np.float32)
        check(lib().dsph_plan_strip_image(self.handle, int(basis), int(strip), out.ctypes.data, int(n.value), ctypes.byref(n)),
              "dsph_plan_strip_image")
        return out.reshape(-1, 9, 16, 4)

    def strip_split(self, N):
        """How a quad-strip forward of ``N`` maps cuts its work (``dsph_plan_strip_split``): (grid, pieces, workgroups per piece,
        rows of the tape of one map)."""
        g, p, w, r = _c_i32(0), _c_i32(0), _c_i32(0), _c_i64(0)
        check(lib().dsph_plan_strip_split(self.handle, int(N), ctypes.byref(g), ctypes.byref(p), ctypes.byref(w), ctypes.byref(r)),
              "dsph_plan_strip_split")
        return int(g.value), int(p.value), int(w.value), int(r.value)

    def workspace_bytes(self, N, Fin, Fout, K, precision=PREC_FP32, algo=ALGO_AUTO):
        return int(lib().dsph_workspace_bytes(self.handle, int(N), int(Fin), int(Fout), int(K), int(precision),
                                              int(algo)))

    def close(self):
        if getattr(self, "_h", None):
            lib().dsph_plan_destroy(self._h)
            self._h = _c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(t):
    return _c_vp(t.data_ptr()) if t is not None else _c_vp()


def _stream_ptr(device):
    import torch

    return _c_vp(torch.cuda.current_stream(device).cuda_stream)


def _check_dev(t, plan, name):
    import torch

    if not t.is_cuda or t.device.index != plan.device:
        raise ValueError(f"{name} must live on cuda:{plan.device}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 tensor")


def _nbytes(t):
    return t.numel() * t.element_size()


def _aligned16(t):
    """``t`` itself when its first element sits on a 16-byte boundary, else a copy in an allocation of its own (which does).
    The fused Chebyshev kernels load x -- and the quad-strip weight gradient dy -- in 16-byte pieces and the C ABI refuses
    such a pointer off alignment (the workspace query has no pointers, so it cannot change the route for one)."""
    import torch

    if t.data_ptr() % 16 == 0:
        return t
    c = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    c.copy_(t)
    assert c.data_ptr() % 16 == 0
    return c


def _fused_x(plan, x, Fin, Fout, K, algo):
    """x for a forward: an aligned copy (``_aligned16``) only where the call takes the fused kernels and they read x itself -- not
    with ALGO_UNFUSED or on a plan / shape the unfused kernels run (they have scalar forms), and not with Fin % 4 != 0, where the
    kernels read a padded copy in the workspace."""
    if algo == ALGO_UNFUSED or Fin % 4 != 0 or x.data_ptr() % 16 == 0 or not plan.fused_ok(Fin, Fout, K):
        return x
    return _aligned16(x)


def _check_out(out, plan, shape, name="out"):
    _check_dev(out, plan, name)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name} has the wrong shape: {tuple(out.shape)}, expected {tuple(shape)}")


def _ensure_workspace(need, device, workspace, floor=0, same_device=False):
    """The caller's scratch buffer when it holds ``need`` bytes (``same_device``: and lives on ``device``), else a new one of
    max(need, floor) bytes: -> (buffer, whether it was replaced)."""
    import torch

    if workspace is not None and _nbytes(workspace) >= need and (not same_device or workspace.device == device):
        return workspace, False
    return torch.empty(max(need, floor), dtype=torch.uint8, device=device), True


def cheb_forward(plan, x, w, bias, K, act=ACT_NONE, precision=PREC_FP32, algo=ALGO_AUTO, workspace=None, out=None,
                 basis=BASIS_CHEBYSHEV, part=PART_ALL, keep_weights=False):
    """y = dsph_poly_forward_ex(...) on torch CUDA tensors; x (N, n_cols, Fin), w (Fin*K, Fout).
    ``part``: PART_ALL, or PART_INTERIOR / PART_BOUNDARY (fused kernel only) to write only the tiles that do not /
    do touch halo rows -- pass the same ``out`` to both calls.
    ``keep_weights``: the caller vouches that ``workspace`` was last used by a call with the same weight values, shape,
    basis and precision (DSPH_FWD_KEEP_WEIGHTS: no weight-preparation launches); dropped when the workspace is replaced.
    Every contiguous float32 tensor is accepted: an ``x`` off 16-byte alignment is replaced by an aligned copy where -- and only
    where -- the call runs on the fused kernels, which the C ABI would refuse (``_fused_x``); w, bias and out need 4 bytes only."""
    import torch

    _check_dev(x, plan, "x")
    _check_dev(w, plan, "w")
    N, rows, Fin = x.shape
    if rows != plan.n_cols:
        raise ValueError(f"x has {rows} rows, the plan multiplies vectors of {plan.n_cols} rows")
    if w.shape[0] != Fin * K:
        raise ValueError(f"w has {w.shape[0]} rows, expected Fin*K = {Fin * K}")
    Fout = int(w.shape[1])
    x = _fused_x(plan, x, int(Fin), Fout, int(K), algo)
    if bias is not None:
        _check_dev(bias, plan, "bias")
        if bias.numel() != Fout:
            raise ValueError("bias must have Fout elements")
    need = plan.workspace_bytes(N, Fin, Fout, K, precision, algo)
    if need > 0:
        workspace, replaced = _ensure_workspace(need, x.device, workspace)
        keep_weights = keep_weights and not replaced
    orows = plan.out_rows
    if out is None:
        out = torch.empty((N, orows, Fout), dtype=torch.float32, device=x.device)
    else:
        _check_out(out, plan, (N, orows, Fout))
    rc = lib().dsph_poly_forward_ex(
        plan.handle, _ptr(x), _ptr(w), _ptr(bias), _ptr(out), int(N), int(Fin), Fout, int(K), int(basis), int(act),
        int(precision), int(algo), int(part), FWD_KEEP_WEIGHTS if (keep_weights and need > 0) else 0,
        _ptr(workspace) if need > 0 else _c_vp(),
        _nbytes(workspace) if need > 0 else 0, _stream_ptr(x.device),
    )
    check(rc, "dsph_poly_forward_ex")
    return out, workspace


def pool_fusable(plan, N, Fin, Fout, K, act=ACT_NONE):
    """Whether ``cheb_forward_pool`` can run this layer on this plan (``dsph_plan_pool_fusable``)."""
    return bool(lib().dsph_plan_pool_fusable(plan.handle, int(N), int(Fin), int(Fout), int(K), int(act)))


def cheb_forward_pool(plan, x, w, bias, K, pool_type=POOL_MAX, act=ACT_NONE, precision=PREC_FP32, workspace=None,
                      basis=BASIS_CHEBYSHEV, keep_weights=False, out=None):
    """pool(act(conv(x) + bias)) with HealpyPool(p = 1) reduced in the kernels' store step (``dsph_poly_forward_pool``):
    -> (y_pooled (N, rows / 4, Fout), workspace).  The full-resolution output is never written.
    An ``x`` off 16-byte alignment is replaced by an aligned copy (``_fused_x``: this call is the fused kernels' only);
    ``out``: the pooled map's tensor, 16-byte aligned (the pooled stores are 16 bytes wide: the C ABI refuses another)."""
    import torch

    _check_dev(x, plan, "x")
    _check_dev(w, plan, "w")
    N, rows, Fin = x.shape
    Fout = int(w.shape[1])
    x = _fused_x(plan, x, int(Fin), Fout, int(K), ALGO_FUSED)
    need = plan.workspace_bytes(N, Fin, Fout, K, precision, ALGO_FUSED)
    if need > 0:
        workspace, replaced = _ensure_workspace(need, x.device, workspace)
        keep_weights = keep_weights and not replaced
    if out is None:
        out = torch.empty((N, rows // 4, Fout), dtype=torch.float32, device=x.device)
    else:
        _check_out(out, plan, (N, rows // 4, Fout))
    rc = lib().dsph_poly_forward_pool(
        plan.handle, _ptr(x), _ptr(w), _ptr(bias), _c_vp(), _ptr(out), int(N), int(Fin), Fout, int(K), int(basis), int(act),
        int(precision), int(pool_type), FWD_KEEP_WEIGHTS if (keep_weights and need > 0) else 0,
        _ptr(workspace) if need > 0 else _c_vp(), _nbytes(workspace) if need > 0 else 0, _stream_ptr(x.device))
    check(rc, "dsph_poly_forward_pool")
    return out, workspace


def cheb_step(plan, inp, prev, alpha, beta, rows=0, out=None):
    """out = alpha * (L~ @ inp) - beta * prev on (N, n_cols, F) planes."""
    import torch

    _check_dev(inp, plan, "in")
    N, r, F = inp.shape
    if r != plan.n_cols:
        raise ValueError("plane row count must equal the plan's n_cols")
    if prev is not None:
        _check_dev(prev, plan, "prev")
    if out is None:
        # rows the step does not produce (halo rows of a shard, rows beyond `rows`) stay zero
        full = plan.n_cols == plan.n_rows and (rows <= 0 or rows == plan.n_rows)
        out = torch.empty_like(inp) if full else torch.zeros_like(inp)
    rc = lib().dsph_cheb_step(plan.handle, _ptr(inp), _ptr(prev), _ptr(out), int(N), int(F), float(alpha),
                              float(beta), int(rows), _stream_ptr(inp.device))
    check(rc, "dsph_cheb_step")
    return out


def cheb_contract(planes, w, bias, rows, K, act=ACT_NONE, precision=PREC_FP32, out=None):
    """Contraction over a list of K (N, plane_rows, Fin) planes -> (N, rows, Fout).  Planes, w, bias and ``out`` (the result's
    tensor) may sit at any 4-byte alignment: the launch picks the kernels' scalar forms per pointer."""
    import torch

    p0 = planes[0]
    N, plane_rows, Fin = p0.shape
    Fout = int(w.shape[1])
    arr = (_c_vp * K)(*[p.data_ptr() for p in planes])
    if out is None:
        out = torch.empty((N, rows, Fout), dtype=torch.float32, device=p0.device)
    elif tuple(out.shape) != (N, rows, Fout) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != p0.device:
        raise ValueError(f"out must be a contiguous float32 ({N}, {rows}, {Fout}) tensor on {p0.device}")
    rc = lib().dsph_cheb_contract(ctypes.cast(arr, _c_vp), int(plane_rows), _ptr(w), _ptr(bias), _ptr(out), int(N),
                                  int(rows), int(Fin), Fout, int(K), int(act), int(precision), p0.device.index,
                                  _stream_ptr(p0.device))
    check(rc, "dsph_cheb_contract")
    return out


def cheb_planes(plan, x, K, basis=BASIS_CHEBYSHEV, algo=ALGO_AUTO, out=None):
    """[x, T_1 x, ..., T_{K-1} x]: the recurrence without the contraction (``dsph_cheb_planes``).
    Every plane has x's shape (N, n_cols, Fin) and is valid on the plan's output rows.
    ``out``: the (K - 1, N, n_cols, Fin) tensor the planes 1 .. K - 1 are written to.  With ALGO_AUTO an ``x`` or ``out`` off
    16-byte alignment runs on the step kernels (the C ABI's choice: no workspace depends on it); with ALGO_FUSED an ``x`` off
    alignment is replaced by an aligned copy and such an ``out`` is refused."""
    import torch

    _check_dev(x, plan, "x")
    if x.dim() != 3 or x.shape[1] != plan.n_cols:
        raise ValueError(f"x must be (N, {plan.n_cols}, Fin), got {tuple(x.shape)}")
    N, M, Fin = x.shape
    if K <= 1:
        return [x]
    if out is None:
        out = torch.empty((K - 1, N, M, Fin), dtype=torch.float32, device=x.device)
    else:
        _check_out(out, plan, (K - 1, N, M, Fin))
    x0 = x
    if algo == ALGO_FUSED:
        x = _aligned16(x)
    rc = lib().dsph_cheb_planes(plan.handle, _ptr(x), _ptr(out), int(N), int(Fin), int(K), int(basis), int(algo),
                                _stream_ptr(x.device))
    check(rc, "dsph_cheb_planes")
    return [x0] + [out[k] for k in range(K - 1)]


def cheb_backward_weights(plan, x, dy, K, basis=BASIS_CHEBYSHEV, algo=ALGO_AUTO, workspace=None, precision=PREC_FP32, out=None):
    """dkernel[f*K + k, o] = sum_{n,m} (T_k x)[n,m,f] dy[n,m,o] (``dsph_cheb_backward_weights``).
    Returns (dkernel, workspace).  ``out``: the (Fin*K, Fout) tensor dkernel is written to (any 4-byte alignment).
    Unless ALGO_UNFUSED is asked for, an ``x`` with Fin % 4 == 0 off 16-byte alignment is replaced by an aligned copy (the fused
    kernels, where the plan has them, would refuse it), and so is such a ``dy`` of the quad-strip gradient's shape (K = 5,
    64 -> 64 j, three-term bf16), which the C ABI would otherwise hand to the slower BFS-tile kernel."""
    import torch

    _check_dev(x, plan, "x")
    _check_dev(dy, plan, "dy")
    N, M, Fin = x.shape
    if M != plan.n_cols or dy.dim() != 3 or dy.shape[0] != N or dy.shape[1] != plan.out_rows:
        raise ValueError(f"x must be (N, {plan.n_cols}, Fin) and dy (N, {plan.out_rows}, Fout)")
    Fout = int(dy.shape[2])
    if algo != ALGO_UNFUSED:
        if Fin % 4 == 0:
            x = _aligned16(x)
        if K == 5 and Fin == 64 and Fout % 64 == 0 and precision == PREC_BF16X3:
            dy = _aligned16(dy)
    need = int(lib().dsph_backward_weights_workspace_bytes(plan.handle, int(N), int(Fin), Fout, int(K), int(algo)))
    workspace, _ = _ensure_workspace(need, x.device, workspace, floor=16, same_device=True)
    if out is None:
        dw = torch.empty((Fin * K, Fout), dtype=torch.float32, device=x.device)
    else:
        _check_out(out, plan, (Fin * K, Fout))
        dw = out
    rc = lib().dsph_cheb_backward_weights(plan.handle, _ptr(x), _ptr(dy), _ptr(dw), int(N), int(Fin), Fout, int(K),
                                          int(basis), int(precision), int(algo), _ptr(workspace),
                                          _nbytes(workspace), _stream_ptr(x.device))
    check(rc, "dsph_cheb_backward_weights")
    return dw, workspace


def cheb_wgrad(planes, dy, rows=None, workspace=None, out=None):
    """dw[f*K + k, o] = sum_{n,m} planes[k][n,m,f] * dy[n,m,o] for a list of K (N, plane_rows, Fin) planes.
    Every pointer may sit at any 4-byte alignment (the kernels read and write by the element); ``out``: dw's tensor."""
    import torch

    p0 = planes[0]
    K = len(planes)
    N, plane_rows, Fin = p0.shape
    rows = int(dy.shape[1]) if rows is None else int(rows)
    Fout = int(dy.shape[2])
    need = int(lib().dsph_wgrad_workspace_bytes(int(N), rows, int(Fin), Fout, K))
    workspace, _ = _ensure_workspace(need, p0.device, workspace)
    if out is None:
        dw = torch.empty((Fin * K, Fout), dtype=torch.float32, device=p0.device)
    elif tuple(out.shape) != (Fin * K, Fout) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != p0.device:
        raise ValueError(f"out must be a contiguous float32 ({Fin * K}, {Fout}) tensor on {p0.device}")
    else:
        dw = out
    arr = (_c_vp * K)(*[p.data_ptr() for p in planes])
    rc = lib().dsph_cheb_wgrad(ctypes.cast(arr, _c_vp), int(plane_rows), _ptr(dy), _ptr(dw), int(N), rows, int(Fin),
                               Fout, K, _ptr(workspace), _nbytes(workspace),
                               p0.device.index, _stream_ptr(p0.device))
    check(rc, "dsph_cheb_wgrad")
    return dw, workspace


def rows_pack(src, idx, out=None):
    """buf[n, i, :] = src[n, idx[i], :]; idx is an int32 CUDA tensor."""
    import torch

    N, rows, F = src.shape
    n_idx = int(idx.numel())
    if out is None:
        out = torch.empty((N, n_idx, F), dtype=torch.float32, device=src.device)
    rc = lib().dsph_rows_pack(_ptr(src), int(rows), _ptr(idx), n_idx, _ptr(out), int(N), int(F), src.device.index,
                              _stream_ptr(src.device))
    check(rc, "dsph_rows_pack")
    return out


def rows_unpack(dst, idx, buf):
    """dst[n, idx[i], :] = buf[n, i, :] in place."""
    N, rows, F = dst.shape
    rc = lib().dsph_rows_unpack(_ptr(dst), int(rows), _ptr(idx), int(idx.numel()), _ptr(buf), int(N), int(F),
                                dst.device.index, _stream_ptr(dst.device))
    check(rc, "dsph_rows_unpack")
    return dst


def residual_epilogue(y, skip, alpha=1.0, act=ACT_NONE, act_before=False):
    """In place, one pass (``dsph_residual_epilogue``): y = act(y + alpha * skip), or act(y) + alpha * skip."""
    if not (y.is_cuda and skip.is_cuda and y.device == skip.device):
        raise ValueError("residual_epilogue works on HIP tensors of one device")
    if y.dtype != skip.dtype or str(y.dtype) != "torch.float32" or y.shape != skip.shape:
        raise ValueError("y and skip must be float32 tensors of one shape")
    if not (y.is_contiguous() and skip.is_contiguous()):
        raise ValueError("y and skip must be contiguous")
    rc = lib().dsph_residual_epilogue(_ptr(y), _ptr(skip), int(y.numel()), float(alpha), int(act), 1 if act_before else 0,
                                      int(y.device.index), _stream_ptr(y.device))
    check(rc, "dsph_residual_epilogue")
    return y


def healpix_pool(x, group, pool_type=POOL_MAX):
    """y[n, m, f] = max | mean over the ``group`` = 4^p consecutive (NEST children) rows of x (``dsph_healpix_pool``)."""
    import torch

    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 3:
        raise ValueError("healpix_pool works on a contiguous float32 (N, rows, F) HIP tensor")
    N, M, F = x.shape
    if M % group != 0:
        raise ValueError(f"{M} rows are not a multiple of the group size {group}")
    y = torch.empty((N, M // group, F), dtype=torch.float32, device=x.device)
    rc = lib().dsph_healpix_pool(_ptr(x), _ptr(y), int(N), int(M // group), int(F), int(group), int(pool_type), x.device.index,
                                 _stream_ptr(x.device))
    check(rc, "dsph_healpix_pool")
    return y


def healpix_pool_backward(x, dy, group, pool_type=POOL_MAX):
    """Gradient of ``healpix_pool`` with respect to its input (``dsph_healpix_pool_backward``)."""
    import torch

    N, Mo, F = dy.shape
    dx = torch.empty((N, Mo * group, F), dtype=torch.float32, device=dy.device)
    rc = lib().dsph_healpix_pool_backward(_ptr(x), _ptr(dy.contiguous()), _ptr(dx), int(N), int(Mo), int(F), int(group),
                                          int(pool_type), dy.device.index, _stream_ptr(dy.device))
    check(rc, "dsph_healpix_pool_backward")
    return dx


REORDER_MAX_NSIDE = 8192  # dsph_healpix_reorder keeps pixel indices in int32


def healpix_reorder(x, nside, to_nest, out=None):
    """The full-sky (N, 12 nside^2, F) map ``x`` in the other pixel ordering (``dsph_healpix_reorder``): ``to_nest`` true takes a
    RING-ordered map to NEST order, false a NEST-ordered one to RING order.  ``out`` must not share memory with ``x``; allocated
    when None.  The arguments are checked before the library or the GPU is touched."""
    import torch

    nside = int(nside)
    if nside < 1 or nside & (nside - 1):
        raise ValueError(f"healpix_reorder: nside = {nside} is not a power of two >= 1")
    if nside > REORDER_MAX_NSIDE:
        raise ValueError(f"healpix_reorder: nside = {nside} is beyond the kernel's limit of {REORDER_MAX_NSIDE} (int32 pixel indices)")
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError("healpix_reorder works on a contiguous float32 (N, 12 nside^2, F) tensor")
    N, M, F = x.shape
    if M != 12 * nside * nside or F < 1:
        raise ValueError(f"healpix_reorder: a map of {M} pixels and {F} channels is not a full sky of nside {nside} "
                         f"({12 * nside * nside} pixels) with at least one channel")
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.is_contiguous()
                                and out.shape == x.shape and out.device == x.device):
        raise ValueError("out must be a contiguous float32 tensor of x's shape on x's device")
    if not x.is_cuda:
        raise ValueError("healpix_reorder works on a HIP tensor")
    require_gpu()
    if out is None:
        out = torch.empty_like(x)
    if N == 0:  # (an empty tensor has no address to hand over)
        return out
    rc = lib().dsph_healpix_reorder(_ptr(x), _ptr(out), int(N), nside, int(F), 1 if to_nest else 0, x.device.index,
                                    _stream_ptr(x.device))
    check(rc, "dsph_healpix_reorder")
    return out


KNN_MAX_NSIDE = 8192  # dsph_healpix_knn keeps pixel indices in int32
KNN_MAX_K = 64  # ... and the neighbours of a row in the lanes of one wave


def healpix_knn(nside, k, indices=None, lut=None, device=None, out=None):
    """The ``k`` nearest pixels of every pixel of a HEALPix map in NEST order (``dsph_healpix_knn``) ->
    ``(nbr int32 [M, k], d2 float64 [M, k], ok uint8 [M])`` on ``device``.

    ``indices``: sorted NEST ids of a partial-sky set, an int64 tensor on the device; None: the full sky, M = 12 nside^2.
    ``lut``: with ``indices``, the int32 table of length 12 nside^2 that maps a NEST id to its row of the set, or -1.
    A row with ``ok = 1`` holds the rows of the k nearest other pixels of the set by chord distance between pixel centres, ascending
    by (d2, row), and their squared chords; the contents of a row with ``ok = 0`` are unspecified (the search window held fewer than
    k pixels of the set, or could not prove the k-th of them nearest: the edge of a footprint).  ``out``: the three tensors to write
    into.  The arguments are checked before the library or the GPU is touched."""
    import torch

    nside, k = int(nside), int(k)
    if nside < 1 or nside & (nside - 1):
        raise ValueError(f"healpix_knn: nside = {nside} is not a power of two >= 1")
    if nside > KNN_MAX_NSIDE:
        raise ValueError(f"healpix_knn: nside = {nside} is beyond the kernel's limit of {KNN_MAX_NSIDE} (int32 pixel indices)")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"healpix_knn: k = {k} neighbours, the kernel takes 1 .. {KNN_MAX_K}")
    npix = 12 * nside * nside
    if (indices is None) != (lut is None):
        raise ValueError("healpix_knn: indices and lut come together (both None: the full sky)")
    if indices is not None:
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int64 and indices.dim() == 1 and indices.is_contiguous()):
            raise ValueError("healpix_knn: indices must be a contiguous int64 tensor [M]")
        if not (isinstance(lut, torch.Tensor) and lut.dtype == torch.int32 and lut.dim() == 1 and lut.is_contiguous()
                and lut.shape[0] == npix):
            raise ValueError(f"healpix_knn: lut must be a contiguous int32 tensor of 12 nside^2 = {npix} entries")
        if lut.device != indices.device:
            raise ValueError(f"healpix_knn: lut lives on {lut.device}, indices on {indices.device}")
        if device is not None and torch.device(device) != indices.device:
            raise ValueError(f"healpix_knn: indices live on {indices.device}, device = {device}")
        dev, M = indices.device, int(indices.shape[0])
    else:
        dev, M = torch.device("cuda" if device is None else device), npix
    if M <= k:
        raise ValueError(f"healpix_knn: a set of M = {M} pixels has no {k} neighbours per pixel (M > k is required)")
    if M > npix or M >= 2**31:
        raise ValueError(f"healpix_knn: M = {M} rows, a map of nside {nside} has at most {min(npix, 2**31 - 1)}")
    if dev.type != "cuda":
        raise ValueError("healpix_knn works on a HIP device")
    require_gpu()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = (torch.empty((M, k), dtype=torch.int32, device=dev), torch.empty((M, k), dtype=torch.float64, device=dev),
               torch.empty((M,), dtype=torch.uint8, device=dev))
    nbr, d2, ok = out
    for t, dt, shape, name in ((nbr, torch.int32, (M, k), "nbr"), (d2, torch.float64, (M, k), "d2"), (ok, torch.uint8, (M,), "ok")):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError(f"healpix_knn: out {name} must be a contiguous {dt} tensor of shape {shape} on {dev}")
    rc = lib().dsph_healpix_knn(nside, k, _ptr(indices), _ptr(lut), M, _ptr(nbr), _ptr(d2), _ptr(ok), dev.index, _stream_ptr(dev))
    check(rc, "dsph_healpix_knn")
    return nbr, d2, ok

DISC_MAX_NSIDE = 8192  # dsph_healpix_disc_count / dsph_healpix_gauss_table keep pixel indices in int32
DISC_MAX_W = 512  # ... and select the entries of a row in the LDS of one workgroup


def _disc_set(what, nside, indices, lut, device):
    """The pixel-set arguments the two disc entry points share, checked: -> (device, M)."""
    import torch

    if nside < 1 or nside & (nside - 1):
        raise ValueError(f"{what}: nside = {nside} is not a power of two >= 1")
    if nside > DISC_MAX_NSIDE:
        raise ValueError(f"{what}: nside = {nside} is beyond the kernel's limit of {DISC_MAX_NSIDE} (int32 pixel indices)")
    npix = 12 * nside * nside
    if (indices is None) != (lut is None):
        raise ValueError(f"{what}: indices and lut come together (both None: the full sky)")
    if indices is not None:
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int64 and indices.dim() == 1 and indices.is_contiguous()):
            raise ValueError(f"{what}: indices must be a contiguous int64 tensor [M]")
        if not (isinstance(lut, torch.Tensor) and lut.dtype == torch.int32 and lut.dim() == 1 and lut.is_contiguous()
                and lut.shape[0] == npix):
            raise ValueError(f"{what}: lut must be a contiguous int32 tensor of 12 nside^2 = {npix} entries")
        if lut.device != indices.device:
            raise ValueError(f"{what}: lut lives on {lut.device}, indices on {indices.device}")
        if device is not None and torch.device(device) != indices.device:
            raise ValueError(f"{what}: indices live on {indices.device}, device = {device}")
        dev, M = indices.device, int(indices.shape[0])
    else:
        dev, M = torch.device("cuda" if device is None else device), npix
    if M < 1 or M > npix or M >= 2**31:
        raise ValueError(f"{what}: M = {M} rows, a map of nside {nside} has 1 .. {min(npix, 2**31 - 1)}")
    return dev, M


def _disc_out(what, out, specs, dev):
    """``out`` (or fresh tensors) for the (name, dtype, shape) of ``specs``, checked; a spec whose name is None stays None."""
    import torch

    if out is None:
        out = tuple(None if name is None else torch.empty(shape, dtype=dt, device=dev) for name, dt, shape in specs)
    if len(out) != len(specs):
        raise ValueError(f"{what}: out takes {len(specs)} tensors")
    for t, (name, dt, shape) in zip(out, specs):
        if name is None:
            if t is not None:
                raise ValueError(f"{what}: out holds a tensor that was not asked for")
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError(f"{what}: out {name} must be a contiguous {dt} tensor of shape {shape} on {dev}")
    return tuple(out)


def healpix_disc_count(nside, r2, indices=None, lut=None, device=None, out=None):
    """How many pixels of the set lie within the squared chord ``r2`` of every pixel of a HEALPix map in NEST order, the pixel
    itself included (``dsph_healpix_disc_count``) -> ``(count int32 [M], ok uint8 [M])`` on ``device``.

    ``r2 = (2 sin(rho / 2))^2`` for a disc of radius ``rho <= pi``.  ``indices``, ``lut``: as for ``healpix_knn`` (the ids in any
    order).  A row with ``ok = 0`` is one whose window could not guarantee the count; the caller counts it.  ``out``: the two
    tensors to write into.  The arguments are checked before the library or the GPU is touched."""
    import torch

    what = "healpix_disc_count"
    nside, r2 = int(nside), float(r2)
    dev, M = _disc_set(what, nside, indices, lut, device)
    if not 0.0 <= r2 <= 4.0:
        raise ValueError(f"{what}: r2 = {r2} is not the squared chord of a radius in [0, pi]")
    if dev.type != "cuda":
        raise ValueError(f"{what} works on a HIP device")
    require_gpu()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    count, ok = _disc_out(what, out, (("count", torch.int32, (M,)), ("ok", torch.uint8, (M,))), dev)
    rc = lib().dsph_healpix_disc_count(nside, r2, _ptr(indices), _ptr(lut), M, _ptr(count), _ptr(ok), dev.index, _stream_ptr(dev))
    check(rc, "dsph_healpix_disc_count")
    return count, ok


def healpix_gauss_table(nside, W, sigma_rad, rho, indices=None, lut=None, device=None, want_raw=False, out=None):
    """The finished kernel table of ``HealpySmoothing`` (``dsph_healpix_gauss_table``) -> ``(cols int32 [M, W], vals float32
    [M, W], raw float32 [M, W] or None, ok uint8 [M])`` on ``device``.

    A row holds the ``W`` nearest pixels of the set, the pixel itself included, selected by (squared chord, row) ascending, its
    columns ascending; ``vals`` the Gaussian weights of standard deviation ``sigma_rad`` normalised to sum 1, ``raw`` (with
    ``want_raw``) the weights before the normalisation.  ``rho``: the radius the search window must cover (the radius ``W`` was
    counted for).  A row with ``ok = 0`` is the caller's to complete.  ``out``: the four tensors to write into (raw None without
    ``want_raw``).  The arguments are checked before the library or the GPU is touched."""
    import torch

    what = "healpix_gauss_table"
    nside, W, sigma_rad, rho = int(nside), int(W), float(sigma_rad), float(rho)
    dev, M = _disc_set(what, nside, indices, lut, device)
    if W < 1:
        raise ValueError(f"{what}: W = {W} entries per row, must be at least 1")
    if W > DISC_MAX_W:
        raise ValueError(f"{what}: W = {W} entries per row, the kernel takes 1 .. {DISC_MAX_W}")
    if M < W:
        raise ValueError(f"{what}: a set of M = {M} pixels has no rows of W = {W} (M >= W is required)")
    if not (sigma_rad > 0.0 and 0.0 < rho <= np.pi):
        raise ValueError(f"{what}: sigma_rad = {sigma_rad}, rho = {rho}: sigma_rad > 0 and 0 < rho <= pi are required")
    if dev.type != "cuda":
        raise ValueError(f"{what} works on a HIP device")
    require_gpu()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    specs = (("cols", torch.int32, (M, W)), ("vals", torch.float32, (M, W)), ("raw" if want_raw else None, torch.float32, (M, W)),
             ("ok", torch.uint8, (M,)))
    cols, vals, raw, ok = _disc_out(what, out, specs, dev)
    rc = lib().dsph_healpix_gauss_table(nside, W, sigma_rad, rho, _ptr(indices), _ptr(lut), M, _ptr(cols), _ptr(vals), _ptr(raw),
                                        _ptr(ok), dev.index, _stream_ptr(dev))
    check(rc, "dsph_healpix_gauss_table")
    return cols, vals, raw, ok


def _rotations(what, rot, device, n_maps):
    """``rot`` checked: a contiguous float64 tensor [3, 3] (``n_maps`` None: only that) or [n_maps, 3, 3] on ``device`` (None: its
    own) -> the number of rotations."""
    import torch

    ok_shape = isinstance(rot, torch.Tensor) and (tuple(rot.shape) == (3, 3)
                                                  or (n_maps is not None and tuple(rot.shape) == (n_maps, 3, 3)))
    if not (ok_shape and rot.dtype == torch.float64 and rot.is_contiguous()):
        raise ValueError(f"{what}: rot must be a contiguous float64 tensor [3, 3]" + ("" if n_maps is None else f" or [N = {n_maps}, 3, 3]"))
    if device is not None and rot.device != device:
        raise ValueError(f"{what}: rot lives on {rot.device}, the maps on {device}")
    return 1 if rot.dim() == 2 else int(rot.shape[0])


def healpix_rotate(x, nside, rot, indices=None, lut=None, out=None):
    """The NEST-ordered scalar maps ``x`` (N, M, F) rotated by bilinear interpolation (``dsph_healpix_rotate``):
    out[n, r, :] = sum_j w_j x[n, row(p_j), :] with the four-pixel stencil of ``healpix.get_interp_weights`` at R^T v(indices[r]).

    ``rot``: float64 [3, 3] (one rotation for the batch) or [N, 3, 3] (one per map), on the maps' device.  ``indices``, ``lut``: the
    pixel set as for ``healpix_knn`` (both None: the full sky, M = 12 nside^2); a source pixel outside the set contributes zero.
    ``out`` must not share memory with ``x``; allocated when None.  The arguments are checked before the library or the GPU is
    touched."""
    import torch

    what = "healpix_rotate"
    nside = int(nside)
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError(f"{what} works on a contiguous float32 (N, M, F) tensor")
    _, M = _disc_set(what, nside, indices, lut, None)
    N, Mx, F = x.shape
    if Mx != M or F < 1:
        raise ValueError(f"{what}: a map of {Mx} pixels and {F} channels does not fit the set of {M} pixels (nside {nside}) with at "
                         "least one channel")
    n_rot = _rotations(what, rot, x.device, int(N))
    if indices is not None and indices.device != x.device:
        raise ValueError(f"{what}: indices live on {indices.device}, the maps on {x.device}")
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.is_contiguous()
                                and out.shape == x.shape and out.device == x.device):
        raise ValueError("out must be a contiguous float32 tensor of x's shape on x's device")
    if not x.is_cuda:
        raise ValueError(f"{what} works on a HIP tensor")
    require_gpu()
    if out is None:
        out = torch.empty_like(x)
    if N == 0:  # (an empty tensor has no address to hand over)
        return out
    rc = lib().dsph_healpix_rotate(_ptr(x), _ptr(out), int(N), nside, int(F), _ptr(rot), n_rot, _ptr(lut), _ptr(indices), M,
                                   x.device.index, _stream_ptr(x.device))
    check(rc, "dsph_healpix_rotate")
    return out


def healpix_interp_table(nside, rot, indices=None, lut=None, device=None):
    """The stencils of ``healpix_rotate`` for ONE rotation ``rot`` (float64 [3, 3] on the device) as a table
    (``dsph_healpix_interp_table``) -> ``(cols int32 [M, 4], vals float32 [M, 4])``: ``ell_smooth(cols, vals, x)`` is the rotation,
    on ``healpix.transpose_table(cols, vals)`` its adjoint.  A source outside the set is (col = the row itself, val = 0).  The
    arguments are checked before the library or the GPU is touched."""
    import torch

    what = "healpix_interp_table"
    nside = int(nside)
    dev, M = _disc_set(what, nside, indices, lut, device)
    if indices is None and device is None and isinstance(rot, torch.Tensor):
        dev = rot.device  # (the full sky brings no device along; the rotation does)
    _rotations(what, rot, None, None)
    if dev.type != "cuda":
        raise ValueError(f"{what} works on a HIP device")
    require_gpu()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if rot.device != dev:
        raise ValueError(f"{what}: rot lives on {rot.device}, the table on {dev}")
    cols = torch.empty((M, 4), dtype=torch.int32, device=dev)
    vals = torch.empty((M, 4), dtype=torch.float32, device=dev)
    rc = lib().dsph_healpix_interp_table(nside, _ptr(rot), _ptr(lut), _ptr(indices), M, _ptr(cols), _ptr(vals), dev.index,
                                         _stream_ptr(dev))
    check(rc, "dsph_healpix_interp_table")
    return cols, vals


SHT_MAX_NSIDE = 2048         # dsph_sht_*: the largest nside the transform takes
SHT_CHUNK_BYTES = 1 << 31    # the compositions' F_m scratch: at most this many bytes at a time (but always one map's worth) ...
SHT_CHUNK_COLS = 16384       # ... and at most this many columns (maps x channels; always one map's worth)
SHT_COL_BLOCK = 8            # columns of a workgroup of the kernels (SH_CB): a trip of whole blocks wastes no lanes


def _sht_shape(what, nside, lmax):
    nside, lmax = int(nside), int(lmax)
    if nside < 1 or nside & (nside - 1):
        raise ValueError(f"{what}: nside = {nside} is not a power of two >= 1")
    if nside > SHT_MAX_NSIDE:
        raise ValueError(f"{what}: nside = {nside} is beyond the transform's limit of {SHT_MAX_NSIDE}")
    if lmax < 0 or lmax > 4 * nside - 1:
        raise ValueError(f"{what}: lmax = {lmax} outside [0, 4 nside - 1 = {4 * nside - 1}]")
    return nside, lmax


def _sht_lmax_of(what, nalm):
    lmax = (int(np.sqrt(8 * int(nalm) + 1)) - 3) // 2
    if (lmax + 1) * (lmax + 2) // 2 != int(nalm):
        raise ValueError(f"{what}: {nalm} coefficients are not (lmax + 1)(lmax + 2) / 2 for any lmax")
    return lmax


def _sht_map(what, x, nside, indices, lut, name="x"):
    """A map argument checked: contiguous float32 (N, M, F) that fits the pixel set -> (N, M, F)."""
    import torch

    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError(f"{what}: {name} must be a contiguous float32 (N, M, F) tensor")
    _, M = _disc_set(what, nside, indices, lut, None)
    N, Mx, F = (int(v) for v in x.shape)
    if Mx != M or F < 1:
        raise ValueError(f"{what}: a map of {Mx} pixels and {F} channels does not fit the set of {M} pixels (nside {nside}) with at "
                         "least one channel")
    if indices is not None and indices.device != x.device:
        raise ValueError(f"{what}: indices live on {indices.device}, the maps on {x.device}")
    return N, M, F


def _sht_out(what, out, src, dtype, shape, name):
    """``out`` (or a fresh tensor) of ``dtype`` and ``shape`` on the device of ``src``, sharing no memory with it."""
    import torch

    if out is None:
        return torch.empty(shape, dtype=dtype, device=src.device)
    if not (isinstance(out, torch.Tensor) and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()
            and out.device == src.device):
        raise ValueError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {src.device} ({name})")
    a0, b0 = src.data_ptr(), out.data_ptr()
    if src.numel() and out.numel() and a0 < b0 + _nbytes(out) and b0 < a0 + _nbytes(src):
        raise ValueError(f"{what}: out shares memory with the input; the transform cannot run in place")
    return out


def _sht_hip(what, t):
    if not t.is_cuda:
        raise ValueError(f"{what} works on a HIP tensor")
    require_gpu()


def sht_fm_shape(nside, lmax, N, F):
    """Shape of the float64 F_m array of ``N`` maps of ``F`` channels: [lmax + 1, 4 nside - 1, N F, 2]."""
    return (int(lmax) + 1, 4 * int(nside) - 1, int(N) * int(F), 2)


def sht_alm_size(lmax):
    return (int(lmax) + 1) * (int(lmax) + 2) // 2


def sht_ring_analysis(x, nside, lmax, indices=None, lut=None, out=None):
    """F_m(ring) = sum_j x[ring, j] e^{-i m phi_j}, m <= lmax, of the NEST maps ``x`` (N, M, F) float32 (``dsph_sht_ring_analysis``) ->
    float64 [lmax + 1, 4 nside - 1, N F, 2].  ``indices``, ``lut``: the footprint as for ``healpix_rotate``; pixels outside it count
    as zero.  The arguments are checked before the library or the GPU is touched."""
    import torch

    what = "sht_ring_analysis"
    nside, lmax = _sht_shape(what, nside, lmax)
    N, M, F = _sht_map(what, x, nside, indices, lut)
    out = _sht_out(what, out, x, torch.float64, sht_fm_shape(nside, lmax, N, F), "F_m")
    _sht_hip(what, x)
    if N == 0:
        return out
    rc = lib().dsph_sht_ring_analysis(_ptr(x), _ptr(out), N, nside, F, lmax, _ptr(lut), _ptr(indices), M, x.device.index,
                                      _stream_ptr(x.device))
    check(rc, "dsph_sht_ring_analysis")
    return out


def _sht_fm(what, fm, nside, lmax, N, F):
    import torch

    shape = sht_fm_shape(nside, lmax, N, F)
    if not (isinstance(fm, torch.Tensor) and fm.dtype == torch.float64 and tuple(fm.shape) == shape and fm.is_contiguous()):
        raise ValueError(f"{what}: fm must be a contiguous float64 tensor of shape {shape}")


def _sht_alm(what, alm, nside):
    import torch

    if not (isinstance(alm, torch.Tensor) and alm.dtype == torch.complex128 and alm.dim() == 3 and alm.is_contiguous()
            and alm.shape[2] >= 1):
        raise ValueError(f"{what}: alm must be a contiguous complex128 (N, nalm, F) tensor with at least one channel")
    lmax = _sht_lmax_of(what, alm.shape[1])
    _sht_shape(what, nside, lmax)
    return int(alm.shape[0]), lmax, int(alm.shape[2])


def sht_legendre_analysis(fm, nside, lmax, N, F, out=None):
    """a_lm = w sum_rings lambda_lm(theta_ring) F_m(ring), w = 4 pi / npix (``dsph_sht_legendre_analysis``): ``fm`` as
    ``sht_ring_analysis`` returns it -> complex128 (N, nalm, F) in healpy's packed layout."""
    import torch

    what = "sht_legendre_analysis"
    nside, lmax = _sht_shape(what, nside, lmax)
    N, F = int(N), int(F)
    if N < 0 or F < 1:
        raise ValueError(f"{what}: N = {N} maps of F = {F} channels")
    _sht_fm(what, fm, nside, lmax, N, F)
    out = _sht_out(what, out, fm, torch.complex128, (N, sht_alm_size(lmax), F), "alm")
    _sht_hip(what, fm)
    if N == 0:
        return out
    rc = lib().dsph_sht_legendre_analysis(_ptr(fm), _ptr(out), N, nside, F, lmax, fm.device.index, _stream_ptr(fm.device))
    check(rc, "dsph_sht_legendre_analysis")
    return out


def sht_legendre_synthesis(alm, nside, out=None):
    """F_m(ring) = sum_l a_lm lambda_lm(theta_ring) (``dsph_sht_legendre_synthesis``): ``alm`` complex128 (N, nalm, F) ->
    float64 [lmax + 1, 4 nside - 1, N F, 2]."""
    import torch

    what = "sht_legendre_synthesis"
    N, lmax, F = _sht_alm(what, alm, int(nside))
    nside = int(nside)
    out = _sht_out(what, out, alm, torch.float64, sht_fm_shape(nside, lmax, N, F), "F_m")
    _sht_hip(what, alm)
    if N == 0:
        return out
    rc = lib().dsph_sht_legendre_synthesis(_ptr(alm), _ptr(out), N, nside, F, lmax, alm.device.index, _stream_ptr(alm.device))
    check(rc, "dsph_sht_legendre_synthesis")
    return out


def sht_ring_synthesis(fm, nside, lmax, N, F, indices=None, lut=None, out=None):
    """map[ring, j] = Re sum_m c_m F_m(ring) e^{+i m phi_j}, c_0 = 1, c_m = 2 (``dsph_sht_ring_synthesis``) -> float32 (N, M, F) in
    NEST order; on a footprint only its rows are written."""
    import torch

    what = "sht_ring_synthesis"
    nside, lmax = _sht_shape(what, nside, lmax)
    N, F = int(N), int(F)
    if N < 0 or F < 1:
        raise ValueError(f"{what}: N = {N} maps of F = {F} channels")
    _sht_fm(what, fm, nside, lmax, N, F)
    _, M = _disc_set(what, nside, indices, lut, None)
    if indices is not None and indices.device != fm.device:
        raise ValueError(f"{what}: indices live on {indices.device}, F_m on {fm.device}")
    out = _sht_out(what, out, fm, torch.float32, (N, M, F), "the maps")
    _sht_hip(what, fm)
    if N == 0:
        return out
    rc = lib().dsph_sht_ring_synthesis(_ptr(fm), _ptr(out), N, nside, F, lmax, _ptr(lut), _ptr(indices), M, fm.device.index,
                                       _stream_ptr(fm.device))
    check(rc, "dsph_sht_ring_synthesis")
    return out


def sht_chunk_maps(nside, lmax, F):
    """Maps per trip of the compositions: the F_m scratch of a trip stays within ``SHT_CHUNK_BYTES`` and ``SHT_CHUNK_COLS`` columns,
    but a trip always holds one whole map; where the limits allow, a count whose columns are a multiple of ``SHT_COL_BLOCK``."""
    per_map = 16 * (int(lmax) + 1) * (4 * int(nside) - 1) * int(F)
    step = max(1, min(SHT_CHUNK_BYTES // per_map, SHT_CHUNK_COLS // int(F)))
    whole = [s for s in range(step, max(step - SHT_COL_BLOCK, 0), -1) if s * int(F) % SHT_COL_BLOCK == 0]
    return whole[0] if whole else step  # (the largest count within the limits whose columns fill the kernels' blocks of 8)


def sht_analysis(x, nside, lmax, indices=None, lut=None, out=None):
    """``sht_legendre_analysis(sht_ring_analysis(x))``, the maps taken ``sht_chunk_maps`` at a time through one scratch array:
    NEST maps (N, M, F) float32 -> complex128 (N, nalm, F), the quadrature with equal weights (healpy's map2alm with iter=0,
    use_weights=False)."""
    import torch

    what = "sht_analysis"
    nside, lmax = _sht_shape(what, nside, lmax)
    N, M, F = _sht_map(what, x, nside, indices, lut)
    out = _sht_out(what, out, x, torch.complex128, (N, sht_alm_size(lmax), F), "alm")
    _sht_hip(what, x)
    step = sht_chunk_maps(nside, lmax, F)
    fm = None
    for n0 in range(0, N, step):
        n1 = min(n0 + step, N)
        if fm is None or n1 - n0 != step:
            fm = torch.empty(sht_fm_shape(nside, lmax, n1 - n0, F), dtype=torch.float64, device=x.device)
        sht_ring_analysis(x[n0:n1], nside, lmax, indices, lut, out=fm)
        sht_legendre_analysis(fm, nside, lmax, n1 - n0, F, out=out[n0:n1])
    return out


def sht_synthesis(alm, nside, indices=None, lut=None, out=None):
    """``sht_ring_synthesis(sht_legendre_synthesis(alm))``, chunked like ``sht_analysis``: complex128 (N, nalm, F) -> NEST maps
    (N, M, F) float32 (healpy's alm2map).  On a footprint only its rows exist."""
    import torch

    what = "sht_synthesis"
    nside = int(nside)
    N, lmax, F = _sht_alm(what, alm, nside)
    _, M = _disc_set(what, nside, indices, lut, None)
    if indices is not None and indices.device != alm.device:
        raise ValueError(f"{what}: indices live on {indices.device}, alm on {alm.device}")
    out = _sht_out(what, out, alm, torch.float32, (N, M, F), "the maps")
    _sht_hip(what, alm)
    step = sht_chunk_maps(nside, lmax, F)
    fm = None
    for n0 in range(0, N, step):
        n1 = min(n0 + step, N)
        if fm is None or n1 - n0 != step:
            fm = torch.empty(sht_fm_shape(nside, lmax, n1 - n0, F), dtype=torch.float64, device=alm.device)
        sht_legendre_synthesis(alm[n0:n1], nside, out=fm)
        sht_ring_synthesis(fm, nside, lmax, n1 - n0, F, indices, lut, out=out[n0:n1])
    return out


def rows_layout(t):
    """Row stride ``ld`` (in elements) of a float32 HIP tensor (N, M, d) whose rows are ``ld >= d`` apart with the maps back to
    back -- a contiguous tensor, or a channel slice of one (a view into a wider projection buffer); ``None`` for any other layout."""
    import torch

    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        return None
    N, M, d = t.shape
    s0, s1, s2 = t.stride()
    if d > 1 and s2 != 1:
        return None
    if M > 1 and s1 < d:
        return None
    ld = s1 if M > 1 else max(s1, d)
    if N > 1 and s0 != M * ld:
        return None
    return int(ld)


def _check_tables(nbr, M, device, name):
    import torch

    if not (isinstance(nbr, torch.Tensor) and nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 tensor [M, W]")
    if nbr.device != device:
        raise ValueError(f"{name} lives on {nbr.device}, the maps on {device}")
    if nbr.shape[0] != M:
        raise ValueError(f"{name} has {nbr.shape[0]} rows, the maps have {M}")


def _qkv_layout(q, k, v, num_heads):
    """-> (common row stride, N, M, d) of the three (N, M, d) maps of an attention call."""
    lds = [rows_layout(t) for t in (q, k, v)]
    if None in lds or len(set(lds)) != 1 or not (q.shape == k.shape == v.shape) or not (q.device == k.device == v.device):
        raise ValueError("q, k, v must be float32 HIP tensors of one shape (N, M, d) on one device, rows one common stride apart")
    N, M, d = q.shape
    if num_heads < 1 or d % num_heads != 0:
        raise ValueError(f"d = {d} is not a multiple of num_heads = {num_heads}")
    return lds[0], N, M, d


def _attention_grad_buffers(q, out, lse, dout, grads, num_heads, pair=False):
    """What both attention backwards take besides q, k, v: -> (out, lse, dout) contiguous and of the forward's shapes, the three
    gradient tensors (allocated when ``grads`` is None), their common row stride and the (N, M, heads) scratch ``delta``.
    ``pair``: ``lse`` is the masked dense attention's (N, M, heads, 2) statistic."""
    import torch

    N, M, d = q.shape
    out, dout = out.contiguous(), dout.contiguous()
    if (tuple(out.shape) != (N, M, d) or tuple(dout.shape) != (N, M, d)
            or tuple(lse.shape) != ((N, M, num_heads, 2) if pair else (N, M, num_heads))):
        raise ValueError("out / dout / lse do not have the forward's shapes")
    if grads is None:
        grads = tuple(torch.empty((N, M, d), dtype=torch.float32, device=q.device) for _ in range(3))
    glds = [rows_layout(t) for t in grads]
    if None in glds or len(set(glds)) != 1 or any(tuple(g.shape) != (N, M, d) for g in grads):
        raise ValueError("dq, dk, dv must be float32 HIP tensors (N, M, d), rows one common stride apart")
    delta = torch.empty((N, M, num_heads), dtype=torch.float32, device=q.device)
    return out, lse.contiguous(), dout, grads, glds[0], delta


def nbr_attention(q, k, v, nbr, num_heads, need_lse=True):
    """Attention over the neighbour table ``nbr`` (int32 [M, W], -1 padded) on (N, M, d) maps (``dsph_nbr_attention_forward``):
    -> (out (N, M, d), lse (N, M, heads) or None).  q, k, v may be channel slices of one wider buffer (``rows_layout``)."""
    import torch

    require_gpu()
    ld, N, M, d = _qkv_layout(q, k, v, num_heads)
    _check_tables(nbr, M, q.device, "nbr")
    out = torch.empty((N, M, d), dtype=torch.float32, device=q.device)
    lse = torch.empty((N, M, num_heads), dtype=torch.float32, device=q.device) if need_lse else None
    rc = lib().dsph_nbr_attention_forward(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(lse), _ptr(nbr), int(nbr.shape[1]),
                                          int(N), int(M), int(num_heads), int(d // num_heads), q.device.index,
                                          _stream_ptr(q.device))
    check(rc, "dsph_nbr_attention_forward")
    return out, lse


def nbr_attention_backward(q, k, v, out, lse, dout, nbr, nbrT, num_heads, grads=None):
    """dq, dk, dv of ``nbr_attention`` (``dsph_nbr_attention_backward``; deterministic).  ``nbrT``: the table of the transposed
    graph.  ``grads``: three tensors to write into (channel slices of one buffer: the gradient of a fused q/k/v projection comes
    out as one tensor); allocated when None."""
    require_gpu()
    ld, N, M, d = _qkv_layout(q, k, v, num_heads)
    _check_tables(nbr, M, q.device, "nbr")
    _check_tables(nbrT, M, q.device, "nbrT")
    out, lse, dout, grads, gld, delta = _attention_grad_buffers(q, out, lse, dout, grads, num_heads)
    rc = lib().dsph_nbr_attention_backward(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(lse), _ptr(dout), _ptr(nbr),
                                           int(nbr.shape[1]), _ptr(nbrT), int(nbrT.shape[1]), _ptr(delta), _ptr(grads[0]),
                                           _ptr(grads[1]), _ptr(grads[2]), gld, int(N), int(M), int(num_heads),
                                           int(d // num_heads), q.device.index, _stream_ptr(q.device))
    check(rc, "dsph_nbr_attention_backward")
    return grads


def attention_mask(mask, N, num_heads, M, device=None):
    """The reference's ``mask`` argument of the dense attention as the kernels' operand: -> (t, (sb, sh, sq)), ``t`` a float32
    tensor (n', h', q', M) with n' in {1, N}, h' in {1, heads}, q' in {1, M} and the last dimension contiguous (moved to ``device``
    when given), and the element strides of its batch, head and query dimensions, 0 for a dimension of size 1: the kernels
    broadcast, nothing of size N heads M M is allocated for a broadcast mask.  Views are kept as views (rows need no alignment).
    A shape that does not broadcast against (N, heads, M, M) raises ValueError naming both shapes; a last dimension of 1 is
    expanded to M here.  bool / int masks are converted to float32.  The mask is not differentiable: one that requires grad raises."""
    import torch

    t = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
    if t.requires_grad:
        raise ValueError("the attention mask is not differentiable (it enters the logits as mask * -1e9): pass mask.detach()")
    full = (int(N), int(num_heads), int(M), int(M))
    shape4 = (1,) * (4 - t.dim()) + tuple(t.shape) if t.dim() <= 4 else None
    if shape4 is None or any(s not in (1, f) for s, f in zip(shape4, full)):
        raise ValueError(f"mask of shape {tuple(t.shape)} does not broadcast against the logits (N, heads, M, M) = {full}")
    t = t.to(dtype=torch.float32) if device is None else t.to(device=device, dtype=torch.float32)
    t = t.reshape(shape4)
    if shape4[3] != full[3]:
        t = t.expand(shape4[:3] + (full[3],)).contiguous()
    elif full[3] > 1 and t.stride(3) != 1:
        t = t.contiguous()
    strides = tuple(0 if t.shape[i] == 1 else int(t.stride(i)) for i in range(3))
    return t, strides


def _mask_operand(mask, N, num_heads, M, device):
    t, strides = attention_mask(mask, N, num_heads, M, device)
    if t.data_ptr() % 4 != 0:
        t = t.contiguous()
    return t, strides


def dense_attention(q, k, v, num_heads, need_lse=True, precision=PREC_FP32, mask=None):
    """Attention of every row over ALL rows of its map on (N, M, d) maps (``dsph_dense_attention_forward_prec``; flash style, no
    logit reaches memory): -> (out (N, M, d), lse (N, M, heads) or None).  q, k, v may be channel slices of one wider buffer
    (``rows_layout``).  ``precision``: PREC_FP32 (exact-fp32 MFMA, every depth), PREC_BF16X6 or PREC_BF16X3 (the bf16 split
    arithmetics, depth 32 and 64; any other depth raises).

    ``mask``: the reference's argument (``attention_mask``), added to the logits as ``mask * -1e9``
    (``dsph_dense_attention_forward_masked``).  The statistic then comes back as the pair (N, M, heads, 2) = (m, log l), which
    ``dense_attention_backward`` takes in place of ``lse`` together with the same mask.  ``mask=None`` runs what it always ran."""
    import torch

    require_gpu()
    ld, N, M, d = _qkv_layout(q, k, v, num_heads)
    out = torch.empty((N, M, d), dtype=torch.float32, device=q.device)
    if mask is not None:
        mk, (sb, sh, sq) = _mask_operand(mask, N, num_heads, M, q.device)
        stat = torch.empty((N, M, num_heads, 2), dtype=torch.float32, device=q.device) if need_lse else None
        rc = lib().dsph_dense_attention_forward_masked(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(stat), _ptr(mk), sb, sh, sq,
                                                       int(N), int(M), int(num_heads), int(d // num_heads), int(precision),
                                                       q.device.index, _stream_ptr(q.device))
        check(rc, "dsph_dense_attention_forward_masked")
        return out, stat
    lse = torch.empty((N, M, num_heads), dtype=torch.float32, device=q.device) if need_lse else None
    rc = lib().dsph_dense_attention_forward_prec(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(lse), int(N), int(M),
                                                 int(num_heads), int(d // num_heads), int(precision), q.device.index,
                                                 _stream_ptr(q.device))
    check(rc, "dsph_dense_attention_forward_prec")
    return out, lse


def dense_attention_backward(q, k, v, out, lse, dout, num_heads, grads=None, precision=PREC_FP32, mask=None):
    """dq, dk, dv of ``dense_attention`` (``dsph_dense_attention_backward_prec``; deterministic, nothing of size M^2 is
    allocated).  ``grads``: three tensors to write into (channel slices of one buffer: the gradient of a fused q/k/v projection
    comes out as one tensor); allocated when None.  ``precision``: as in ``dense_attention``.  ``mask``: the forward's, with the
    forward's pair statistic as ``lse`` (``dsph_dense_attention_backward_masked``)."""
    require_gpu()
    ld, N, M, d = _qkv_layout(q, k, v, num_heads)
    if mask is not None:
        mk, (sb, sh, sq) = _mask_operand(mask, N, num_heads, M, q.device)
        out, stat, dout, grads, gld, delta = _attention_grad_buffers(q, out, lse, dout, grads, num_heads, pair=True)
        rc = lib().dsph_dense_attention_backward_masked(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(stat), _ptr(mk), sb, sh, sq,
                                                        _ptr(dout), _ptr(delta), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), gld,
                                                        int(N), int(M), int(num_heads), int(d // num_heads), int(precision),
                                                        q.device.index, _stream_ptr(q.device))
        check(rc, "dsph_dense_attention_backward_masked")
        return grads
    out, lse, dout, grads, gld, delta = _attention_grad_buffers(q, out, lse, dout, grads, num_heads)
    rc = lib().dsph_dense_attention_backward_prec(_ptr(q), _ptr(k), _ptr(v), ld, _ptr(out), _ptr(lse), _ptr(dout),
                                                  _ptr(delta), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), gld, int(N),
                                                  int(M), int(num_heads), int(d // num_heads), int(precision), q.device.index,
                                                  _stream_ptr(q.device))
    check(rc, "dsph_dense_attention_backward_prec")
    return grads


def ell_smooth(cols, vals, x, out=None, reps=None, pass_index=0, mask=None):
    """One smoothing pass of the [M, W] table (int32 ``cols``, float32 ``vals``) over the (N, M, C) map ``x``
    (``dsph_ell_smooth``): out[n, m, c] = sum_j vals[m, j] x[n, cols[m, j], c] for the channels with ``reps[c] > pass_index``
    (all of them when ``reps`` is None; ``reps``: int32 [C] on the device), x[n, m, c] for the others, times ``mask`` ([M, 1] or
    [M, C]) when one is given.  ``out`` must not share memory with ``x``; allocated when None."""
    import torch

    require_gpu()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError("ell_smooth works on a contiguous float32 (N, M, C) HIP tensor")
    N, M, C = x.shape
    _check_tables(cols, M, x.device, "cols")
    if not (vals.dtype == torch.float32 and vals.is_contiguous() and vals.shape == cols.shape and vals.device == x.device):
        raise ValueError("vals must be a contiguous float32 tensor of cols' shape on the maps' device")
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise ValueError("out must be a contiguous float32 HIP tensor of x's shape on x's device")
    if reps is not None and not (reps.dtype == torch.int32 and reps.is_contiguous() and reps.numel() == C and reps.device == x.device):
        raise ValueError(f"reps must be a contiguous int32 tensor of C = {C} elements on the maps' device")
    mask_C = 1
    if mask is not None:
        if not (mask.dtype == torch.float32 and mask.is_contiguous() and mask.dim() == 2 and mask.shape[0] == M
                and mask.device == x.device):
            raise ValueError(f"mask must be a contiguous float32 tensor [M = {M}, 1 or C] on the maps' device")
        mask_C = int(mask.shape[1])
    rc = lib().dsph_ell_smooth(_ptr(cols), _ptr(vals), int(M), int(cols.shape[1]), _ptr(x), _ptr(out), int(N), int(C), _ptr(reps),
                               int(pass_index), _ptr(mask), mask_C, x.device.index, _stream_ptr(x.device))
    check(rc, "dsph_ell_smooth")
    return out


def basis_change(w, coeff, transpose=False, out=None):
    """The weights ``w`` [Fin * Kp, Fout] (row index f * Kp + i) in another polynomial basis (``dsph_basis_change``):
    out[f*Kp + j, o] = sum_i coeff[i, j] w[f*Kp + i, o], or with ``transpose`` sum_i coeff[j, i] w[f*Kp + i, o] -- the map a weight
    gradient takes back.  ``coeff``: float32 [Kp, Kp] on w's device.  ``out`` must not share memory with ``w``; allocated when
    None.  One launch on the current stream, nothing else: it can be captured into a graph."""
    import torch

    require_gpu()
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous()):
        raise ValueError("basis_change works on a contiguous float32 [Fin * Kp, Fout] HIP tensor")
    if not (isinstance(coeff, torch.Tensor) and coeff.dtype == torch.float32 and coeff.dim() == 2 and coeff.is_contiguous()
            and coeff.shape[0] == coeff.shape[1] and coeff.device == w.device):
        raise ValueError("coeff must be a contiguous square float32 tensor [Kp, Kp] on the weights' device")
    Kp = int(coeff.shape[0])
    if Kp < 1 or w.shape[0] % Kp != 0:
        raise ValueError(f"w has {w.shape[0]} rows, not a multiple of Kp = {Kp}")
    if out is None:
        out = torch.empty_like(w)
    elif not (out.is_cuda and out.device == w.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == w.shape):
        raise ValueError("out must be a contiguous float32 HIP tensor of w's shape on w's device")
    rc = lib().dsph_basis_change(_ptr(w), _ptr(coeff), _ptr(out), int(w.shape[0] // Kp), int(w.shape[1]), Kp, 1 if transpose else 0,
                                 w.device.index, _stream_ptr(w.device))
    check(rc, "dsph_basis_change")
    return out


def bn_workspace_bytes(rows, F):
    """Bytes of scratch ``bn_stats`` and ``bn_backward`` need for a (rows, F) map (``dsph_bn_workspace_bytes``): a function of the
    shape alone, 16 F (P + 1) with P = max(1, min(2048, rows, ceil(rows F / 8192)))."""
    return int(lib().dsph_bn_workspace_bytes(int(rows), int(F)))


def _map_rows(t, name, like=None, min_dim=2):
    """-> (rows, channels) of the channels-last map ``t`` (..., C); ``like``: the map whose shape and device it must have."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= min_dim and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 (..., channels) HIP tensor of at least {min_dim} dimensions")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name} must have x's shape and device")
    C = int(t.shape[-1])
    return t.numel() // max(C, 1), C


def _channel_vec(t, F, device, name):
    import torch

    if t is None:
        return
    if not (isinstance(t, torch.Tensor) and t.device == device and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == F):
        raise ValueError(f"{name} must be a contiguous float32 tensor of F = {F} elements on the map's device")


def bn_stats(y, eps, running_mean=None, running_var=None, momentum=0.0, workspace=None):
    """Per-channel batch statistics of the channels-last map ``y`` (..., F) over all its rows (``dsph_bn_stats``): -> (stats,
    workspace) with ``stats`` a float32 [5, F] tensor of mean, biased variance, rstd = 1 / sqrt(var + eps) and what the fp32 mean and
    rstd rounded away of their float64 values (rows 3 and 4: ``bn_backward`` takes them).  ``running_mean`` /
    ``running_var`` ([F], optional) are updated in place on the device the way ``torch.nn.BatchNorm1d`` does (unbiased variance).
    Two launches on the current stream, nothing else."""
    import torch

    require_gpu()
    rows, F = _map_rows(y, "y")
    _channel_vec(running_mean, F, y.device, "running_mean")
    _channel_vec(running_var, F, y.device, "running_var")
    workspace, _ = _ensure_workspace(bn_workspace_bytes(rows, F), y.device, workspace, floor=16, same_device=True)
    stats = torch.empty((5, F), dtype=torch.float32, device=y.device)
    rc = lib().dsph_bn_stats(_ptr(y), rows, F, float(eps), _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(stats[3]), _ptr(stats[4]), _ptr(running_mean),
                             _ptr(running_var), float(momentum), _ptr(workspace), _nbytes(workspace),
                             y.device.index, _stream_ptr(y.device))
    check(rc, "dsph_bn_stats")
    return stats, workspace


def bn_apply(y, mean, rstd, gamma=None, shift=None, act=ACT_NONE, out=None):
    """out = act((y - mean) * rstd * gamma + shift) per channel of the channels-last map ``y`` (``dsph_bn_apply``); ``gamma`` /
    ``shift`` None mean 1 / 0; ``out`` may be ``y`` itself (in place), allocated when None.  One launch on the current stream."""
    import torch

    require_gpu()
    rows, F = _map_rows(y, "y")
    for t, name in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (shift, "shift")):
        _channel_vec(t, F, y.device, name)
    if mean is None or rstd is None:
        raise ValueError("mean and rstd are required")
    if out is None:
        out = torch.empty_like(y)
    elif out is not y and (_map_rows(out, "out") != (rows, F) or out.device != y.device):
        raise ValueError("out must have y's shape and device")
    rc = lib().dsph_bn_apply(_ptr(y), _ptr(out), rows, F, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(shift), int(act), y.device.index,
                             _stream_ptr(y.device))
    check(rc, "dsph_bn_apply")
    return out


def bn_backward(y, z, dz, mean, rstd, gamma=None, act=ACT_NONE, want_dgamma=True, want_dshift=True, workspace=None, mean_lo=None,
                rstd_lo=None):
    """Gradients of ``bn_stats`` + ``bn_apply`` (``dsph_bn_backward``): -> (dy, dgamma or None, dshift or None, workspace) from the
    forward's input ``y``, output ``z`` (None with ACT_NONE) and the upstream gradient ``dz``.  ``mean_lo`` / ``rstd_lo``: rows 3 and 4
    of ``bn_stats``' result (the float64 statistics' low parts; None: the fp32 arrays as they are).  Deterministic; three launches."""
    import torch

    require_gpu()
    rows, F = _map_rows(y, "y")
    if _map_rows(dz, "dz") != (rows, F) or dz.device != y.device:
        raise ValueError("dz must have y's shape and device")
    if act != ACT_NONE and (z is None or _map_rows(z, "z") != (rows, F) or z.device != y.device):
        raise ValueError("z (the forward's output, y's shape) is needed for the activation's derivative")
    for t, name in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (mean_lo, "mean_lo"), (rstd_lo, "rstd_lo")):
        _channel_vec(t, F, y.device, name)
    workspace, _ = _ensure_workspace(bn_workspace_bytes(rows, F), y.device, workspace, floor=16, same_device=True)
    dy = torch.empty_like(y)
    dgamma = torch.empty(F, dtype=torch.float32, device=y.device) if want_dgamma else None
    dshift = torch.empty(F, dtype=torch.float32, device=y.device) if want_dshift else None
    rc = lib().dsph_bn_backward(_ptr(y), _ptr(z if act != ACT_NONE else None), _ptr(dz), _ptr(mean), _ptr(rstd), _ptr(mean_lo), _ptr(rstd_lo), _ptr(gamma), _ptr(dy),
                                _ptr(dgamma), _ptr(dshift), rows, F, int(act), _ptr(workspace),
                                _nbytes(workspace), y.device.index, _stream_ptr(y.device))
    check(rc, "dsph_bn_backward")
    return dy, dgamma, dshift, workspace


LN_MAX_D = 1024  # the widest row the layer-norm kernels hold in registers (csrc/layer_norm.hip)


def ln_workspace_bytes(rows, d):
    """Bytes of scratch ``ln_backward`` needs for the parameter gradients of a (rows, d) map (``dsph_ln_workspace_bytes``): a
    function of the shape alone, 16 d P with P = max(1, min(2048, ceil(rows / 4), ceil(rows d / 8192))); 0 for rows = 0."""
    return int(lib().dsph_ln_workspace_bytes(int(rows), int(d)))


def ln_forward(x, gamma, beta, eps, res=None, out=None, sum_out=None):
    """Layer norm over the trailing axis of ``x`` (..., d), the residual add in front fused (``dsph_ln_forward``): without ``res``
    -> z = LN(x) * gamma + beta; with ``res`` (x's shape) -> (z, sum) with sum = x + res and z = LN(sum) * gamma + beta.  ``gamma`` /
    ``beta``: [d] or None (1 / 0).  ``out``: where z goes (allocated when None); ``sum_out``: where the sum goes -- ``x`` or ``res``
    themselves for in place, allocated when None.  One launch on the current stream."""
    import torch

    require_gpu()
    rows, d = _map_rows(x, "x", min_dim=1)
    _channel_vec(gamma, d, x.device, "gamma")
    _channel_vec(beta, d, x.device, "beta")
    if res is not None:
        _map_rows(res, "res", x, min_dim=1)
        if sum_out is None:
            sum_out = torch.empty_like(x)
        else:
            _map_rows(sum_out, "sum_out", x, min_dim=1)
    elif sum_out is not None:
        raise ValueError("sum_out without res")
    if out is None:
        out = torch.empty_like(x)
    else:
        _map_rows(out, "out", x, min_dim=1)
    if rows:  # (a map without rows has no address to pass)
        rc = lib().dsph_ln_forward(_ptr(x), _ptr(res), _ptr(sum_out), _ptr(out), rows, d, float(eps), _ptr(gamma), _ptr(beta), x.device.index,
                                   _stream_ptr(x.device))
        check(rc, "dsph_ln_forward")
    return out if res is None else (out, sum_out)


def ln_backward(a, dz, gamma, eps, dsum=None, want_dgamma=True, want_dbeta=True, workspace=None):
    """Gradients of ``ln_forward`` (``dsph_ln_backward``): -> (da, dgamma or None, dbeta or None, workspace) from the forward's
    normalised input ``a`` (its sum output, or x when there was no res), the gradient ``dz`` of z and the gradient ``dsum`` that
    reached the sum output (None: none).  ``da`` is the gradient of x and of res alike.  Deterministic; two launches (one when no
    parameter gradient is wanted)."""
    import torch

    require_gpu()
    rows, d = _map_rows(a, "a", min_dim=1)
    _map_rows(dz, "dz", a, min_dim=1)
    if dsum is not None:
        _map_rows(dsum, "dsum", a, min_dim=1)
    _channel_vec(gamma, d, a.device, "gamma")
    if want_dgamma or want_dbeta:
        workspace, _ = _ensure_workspace(ln_workspace_bytes(rows, d), a.device, workspace, floor=16, same_device=True)
    da = torch.empty_like(a)
    new = torch.zeros if rows == 0 else torch.empty  # (the sums over no rows are zero)
    dgamma = new(d, dtype=torch.float32, device=a.device) if want_dgamma else None
    dbeta = new(d, dtype=torch.float32, device=a.device) if want_dbeta else None
    if rows:  # (a map without rows has no address to pass)
        rc = lib().dsph_ln_backward(_ptr(a), _ptr(dz), _ptr(dsum), _ptr(gamma), float(eps), _ptr(da), _ptr(dgamma), _ptr(dbeta), rows, d,
                                    _ptr(workspace), 0 if workspace is None else _nbytes(workspace),
                                    a.device.index, _stream_ptr(a.device))
        check(rc, "dsph_ln_backward")
    return da, dgamma, dbeta, workspace


PATCH_MAX_DIM = 4096  # the longest contraction and the widest output row of the patch GEMM (csrc/patch_gemm.hip)


def _patch_map(t, name, like=None):
    """-> (R, C) of the contiguous float32 (R, C) HIP matrix ``t``; ``like``: the matrix whose shape and device it must have."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 (rows, columns) HIP tensor")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name} must have {tuple(like.shape)} elements on {like.device}")
    return int(t.shape[0]), int(t.shape[1])


def _patch_period(C, P):
    if P < 1 or C % P != 0:
        raise ValueError(f"the bias period P = {P} must be at least 1 and divide the {C} columns")


def patch_gemm(x2d, w, bias, P, act=ACT_NONE, precision=PREC_BF16X6, out=None):
    """out[r, c] = act(sum_j x2d[r, j] w[j, c] + bias[c mod P]) (``dsph_patch_gemm``): the row GEMM of the pseudo-convolutions, bias
    and activation in its store.  ``x2d`` (R, Kd), ``w`` (Kd, C), ``bias`` [P] or None, ``out`` (R, C), allocated when None.  Kd and
    C at most PATCH_MAX_DIM.  One launch on the current stream."""
    import torch

    require_gpu()
    R, Kd = _patch_map(x2d, "x2d")
    Kw, C = _patch_map(w, "w")
    if w.device != x2d.device or Kw != Kd:
        raise ValueError(f"w must be a ({Kd}, C) matrix on x2d's device")
    if R < 1 or not (1 <= Kd <= PATCH_MAX_DIM and 1 <= C <= PATCH_MAX_DIM):
        raise ValueError(f"R = {R}, Kd = {Kd}, C = {C}: at least one row, Kd and C in [1, {PATCH_MAX_DIM}]")
    _patch_period(C, int(P))
    _channel_vec(bias, int(P), x2d.device, "bias")
    if out is None:
        out = torch.empty((R, C), dtype=torch.float32, device=x2d.device)
    elif _patch_map(out, "out") != (R, C) or out.device != x2d.device:
        raise ValueError(f"out must be a ({R}, {C}) matrix on x2d's device")
    rc = lib().dsph_patch_gemm(_ptr(x2d), _ptr(w), _ptr(bias), _ptr(out), R, Kd, C, int(P), int(act), int(precision), x2d.device.index,
                               _stream_ptr(x2d.device))
    check(rc, "dsph_patch_gemm")
    return out


def patch_backward_workspace_bytes(R, C, P):
    """Bytes of scratch ``patch_epilogue_backward`` needs for the bias gradient of an (R, C) map with bias period P
    (``dsph_patch_backward_workspace_bytes``): a function of the shape alone, 8 P max(1, min(2048, ceil(R C / 8192)))."""
    return int(lib().dsph_patch_backward_workspace_bytes(int(R), int(C), int(P)))


def patch_epilogue_backward(y, dy, P, act=ACT_NONE, want_dbias=True, out=None, workspace=None):
    """dz = dy * act'(y), dbias[o] = sum of dz over the rows and the columns = o mod P (``dsph_patch_epilogue_backward``): ->
    (dz, dbias or None, workspace).  ``y``: the forward's output (None with ACT_NONE); ``out``: where dz goes -- ``dy`` itself for
    in place, allocated when None.  Deterministic; two launches (one when no bias gradient is wanted)."""
    import torch

    require_gpu()
    R, C = _patch_map(dy, "dy")
    if R < 1 or not 1 <= C <= PATCH_MAX_DIM:
        raise ValueError(f"R = {R}, C = {C}: at least one row, C in [1, {PATCH_MAX_DIM}]")
    _patch_period(C, int(P))
    if act != ACT_NONE:
        if y is None:
            raise ValueError("y (the forward's output) is needed for the activation's derivative")
        _patch_map(y, "y", dy)
    if out is None:
        out = torch.empty_like(dy)
    elif out is not dy:
        _patch_map(out, "out", dy)
    dbias = None
    if want_dbias:
        workspace, _ = _ensure_workspace(patch_backward_workspace_bytes(R, C, P), dy.device, workspace, floor=16, same_device=True)
        dbias = torch.empty(int(P), dtype=torch.float32, device=dy.device)
    rc = lib().dsph_patch_epilogue_backward(_ptr(y if act != ACT_NONE else None), _ptr(dy), _ptr(out), _ptr(dbias), R, C, int(P), int(act),
                                            _ptr(workspace if want_dbias else None), _nbytes(workspace) if want_dbias else 0,
                                            dy.device.index, _stream_ptr(dy.device))
    check(rc, "dsph_patch_epilogue_backward")
    return out, dbias, workspace
