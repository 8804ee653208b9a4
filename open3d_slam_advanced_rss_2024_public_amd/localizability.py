"""Localizability of the scan-to-map ICP (include/localizability/o3s_localizability.h): which directions of the pose the kept pairs
of the last iteration constrained, and a pose that takes the ICP's correction in those directions only.

    params = LocalizabilityParams(sum_all_min=..., sum_strong_min=..., sum_partial_min=...)   # calibrated, no defaults
    loc = icp.localizability(params)                 # after a successful compute: four launches, one round trip
    T = remap_pose(loc, T_prior, T_icp)              # host arithmetic: the prior stays in the directions of category 0

The three sums are absolute: they scale with the number of kept pairs.  Calibrate them by running the analysis (the mapper's
``Report`` policy) on a well-constrained recording and reading ``sum_all`` / ``sum_strong``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib

LOCALIZABLE, PARTIALLY, NOT_LOCALIZABLE = 2, 1, 0

# the mapper's degeneracyPolicy (cpp/o3s_mapper.hpp, DegeneracyPolicy)
OFF, REPORT, REMAP, CONSTRAIN = "Off", "Report", "Remap", "Constrain"
POLICIES = (OFF, REPORT, REMAP, CONSTRAIN)

# o3s_icp_set_degeneracy's modes (include/degeneracy/o3s_degeneracy.h)
DEGENERACY_OFF, DEGENERACY_FIXED, DEGENERACY_ANALYSE = 0, 1, 2


class LocalizabilityParamsC(C.Structure):   # o3s_localizability_params
    _fields_ = [("filter_min", C.c_double), ("strong_min", C.c_double), ("sum_all_min", C.c_double), ("sum_strong_min", C.c_double),
                ("sum_partial_min", C.c_double)]


class LocalizabilityC(C.Structure):   # o3s_localizability
    _fields_ = [("eval", C.c_double * 6), ("evec", (C.c_double * 3) * 6), ("sum_all", C.c_double * 6), ("sum_strong", C.c_double * 6),
                ("n_strong", C.c_int64 * 6), ("category", C.c_int32 * 6), ("kept", C.c_int64), ("centre", C.c_double * 3), ("gpu_ms", C.c_float),
                ("reserved", C.c_int32)]


class DegeneracySetC(C.Structure):   # o3s_degeneracy_set
    _fields_ = [("n_rot", C.c_int32), ("n_trans", C.c_int32), ("rot", (C.c_double * 3) * 3), ("trans", (C.c_double * 3) * 3)]


class DegeneracyConfigC(C.Structure):   # o3s_degeneracy_config
    _fields_ = [("mode", C.c_int32), ("min_category", C.c_int32), ("fixed_set", DegeneracySetC), ("loc_params", LocalizabilityParamsC)]


class DegeneracyPartialC(C.Structure):   # o3s_degeneracy_partial (include/degeneracy/o3s_degeneracy_partial.h)
    _fields_ = [("num", C.c_double * 6), ("den", C.c_double * 6), ("value", C.c_double * 6), ("category", C.c_int32 * 6),
                ("partial_mask", C.c_int32), ("constrained_mask", C.c_int32)]


@dataclass
class DegeneracyPartial:
    """o3s_degeneracy_partial: the strong-pair sums of the six directions (the mask's order: translation 0..2, rotation 3..5),
    value = -num / den, the categories, the directions of category 1 and the whole constrained set."""
    num: np.ndarray = field(default_factory=lambda: np.zeros(6))
    den: np.ndarray = field(default_factory=lambda: np.zeros(6))
    value: np.ndarray = field(default_factory=lambda: np.zeros(6))
    category: np.ndarray = field(default_factory=lambda: np.zeros(6, np.int32))
    partial_mask: int = 0
    constrained_mask: int = 0

    @classmethod
    def from_c(cls, c: DegeneracyPartialC) -> "DegeneracyPartial":
        return cls(np.array(c.num[:], np.float64), np.array(c.den[:], np.float64), np.array(c.value[:], np.float64),
                   np.array(c.category[:], np.int32), int(c.partial_mask), int(c.constrained_mask))


@dataclass
class DegeneracySet:
    """o3s_degeneracy_set: up to three unit rotation directions and up to three unit translation directions, (n, 3) float64 each,
    mutually orthogonal inside a group.  The ICP step is solved with no component along any of them."""
    rot: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    trans: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))

    def to_c(self) -> DegeneracySetC:
        r = np.asarray(self.rot, np.float64).reshape(-1, 3)
        t = np.asarray(self.trans, np.float64).reshape(-1, 3)
        c = DegeneracySetC()
        c.n_rot, c.n_trans = r.shape[0], t.shape[0]   # (the library refuses a count outside 0..3)
        for j in range(min(r.shape[0], 3)):
            for k in range(3):
                c.rot[j][k] = float(r[j, k])
        for j in range(min(t.shape[0], 3)):
            for k in range(3):
                c.trans[j][k] = float(t[j, k])
        return c

    @classmethod
    def from_c(cls, c: DegeneracySetC) -> "DegeneracySet":
        return cls(np.array([list(c.rot[j]) for j in range(c.n_rot)], np.float64).reshape(-1, 3),
                   np.array([list(c.trans[j]) for j in range(c.n_trans)], np.float64).reshape(-1, 3))


@dataclass
class LocalizabilityParams:
    """o3s_localizability_params.  filter_min / strong_min default to cos 80 deg / cos 35 deg; the three sums have no default."""
    filter_min: float = math.cos(math.radians(80.0))
    strong_min: float = math.cos(math.radians(35.0))
    sum_all_min: float = float("nan")
    sum_strong_min: float = float("nan")
    sum_partial_min: float = float("nan")

    def to_c(self) -> LocalizabilityParamsC:
        return LocalizabilityParamsC(float(self.filter_min), float(self.strong_min), float(self.sum_all_min), float(self.sum_strong_min),
                                     float(self.sum_partial_min))


@dataclass
class Localizability:
    """o3s_localizability: rows 0..2 the translation directions, 3..5 the rotation directions, eigenvalues ascending in each block."""
    eval: np.ndarray = field(default_factory=lambda: np.zeros(6))
    evec: np.ndarray = field(default_factory=lambda: np.zeros((6, 3)))
    sum_all: np.ndarray = field(default_factory=lambda: np.zeros(6))
    sum_strong: np.ndarray = field(default_factory=lambda: np.zeros(6))
    n_strong: np.ndarray = field(default_factory=lambda: np.zeros(6, np.int64))
    category: np.ndarray = field(default_factory=lambda: np.zeros(6, np.int32))
    kept: int = 0
    centre: np.ndarray = field(default_factory=lambda: np.zeros(3))
    gpu_ms: float = 0.0

    @classmethod
    def from_c(cls, c: LocalizabilityC) -> "Localizability":
        return cls(np.array(c.eval[:], np.float64), np.array([list(r) for r in c.evec], np.float64), np.array(c.sum_all[:], np.float64),
                   np.array(c.sum_strong[:], np.float64), np.array(c.n_strong[:], np.int64), np.array(c.category[:], np.int32), int(c.kept),
                   np.array(c.centre[:], np.float64), float(c.gpu_ms))

    def to_c(self) -> LocalizabilityC:
        c = LocalizabilityC()
        for j in range(6):
            c.eval[j], c.sum_all[j], c.sum_strong[j] = float(self.eval[j]), float(self.sum_all[j]), float(self.sum_strong[j])
            c.n_strong[j], c.category[j] = int(self.n_strong[j]), int(self.category[j])
            for k in range(3):
                c.evec[j][k] = float(self.evec[j][k])
        c.kept = int(self.kept)
        for k in range(3):
            c.centre[k] = float(self.centre[k])
        c.gpu_ms = float(self.gpu_ms)
        return c


def _bind(L):
    """Declares the argtypes of the localizability and degeneracy calls on library `L`, once."""
    if _lib.needs_binding(L, __name__):
        pp, op, dp = C.POINTER(LocalizabilityParamsC), C.POINTER(LocalizabilityC), C.POINTER(C.c_double)
        fp = C.POINTER(C.c_float)
        L.o3s_localizability_default_params.argtypes = [pp]
        L.o3s_localizability_default_params.restype = None
        L.o3s_icp_localizability.argtypes = [C.c_void_p, pp, op]
        L.o3s_localizability_estimate.argtypes = [C.c_void_p, fp, fp, C.c_int64, pp, op]
        L.o3s_localizability_remap.argtypes = [op, C.c_int32, dp, dp, dp, C.POINTER(C.c_int32)]
        sp, cp, ip = C.POINTER(DegeneracySetC), C.POINTER(DegeneracyConfigC), C.POINTER(C.c_int32)
        L.o3s_degeneracy_default_config.argtypes = [cp]
        L.o3s_degeneracy_default_config.restype = None
        L.o3s_icp_set_degeneracy.argtypes = [C.c_void_p, C.c_int32, sp, pp, C.c_int32]
        L.o3s_icp_get_degeneracy.argtypes = [C.c_void_p, cp, sp]
        L.o3s_icp_degeneracy_trace.argtypes = [C.c_void_p, ip, C.c_int32]
        L.o3s_icp_degeneracy_trace.restype = C.c_int32
        L.o3s_icp_minimize_degeneracy.argtypes = [C.c_void_p, fp, ip, fp, fp, C.c_int64, sp, fp, fp, fp, fp]
        qp = C.POINTER(DegeneracyPartialC)   # o3s_degeneracy_partial.h (the link names abbreviate "degeneracy")
        L.o3s_icp_set_degen_partial.argtypes = [C.c_void_p, C.c_int32]
        L.o3s_icp_get_degen_partial.argtypes = [C.c_void_p, ip, qp]
        L.o3s_icp_degen_partial_trace.argtypes = [C.c_void_p, ip, dp, C.c_int32]
        L.o3s_icp_degen_partial_trace.restype = C.c_int32
        L.o3s_degen_partial_estimate.argtypes = [C.c_void_p, fp, fp, fp, C.c_int64, pp, op, qp]
        L.o3s_icp_minimize_degen_values.argtypes = [C.c_void_p, fp, ip, fp, fp, C.c_int64, sp, dp, dp, fp, fp, fp, fp]
    return L


def _L():
    return _bind(_lib.lib())


def default_params() -> LocalizabilityParams:
    """o3s_localizability_default_params: the library's own defaults (the three sums NaN)."""
    c = LocalizabilityParamsC()
    _L().o3s_localizability_default_params(C.byref(c))
    return LocalizabilityParams(c.filter_min, c.strong_min, c.sum_all_min, c.sum_strong_min, c.sum_partial_min)


def remap_pose(loc: Localizability, T_prior, T_icp, min_category: int = PARTIALLY):
    """o3s_localizability_remap: (T_out 4 x 4 float64, number of directions replaced by the prior).  With nothing replaced T_out is
    T_icp bit for bit.  Raises ValueError when the library refuses the arguments (min_category outside {1, 2}, a non-finite matrix,
    a correction of pi / 2 or more)."""
    dp = C.POINTER(C.c_double)
    P = np.ascontiguousarray(np.asarray(T_prior, np.float64).T).reshape(16)
    Q = np.ascontiguousarray(np.asarray(T_icp, np.float64).T).reshape(16)
    out = np.zeros(16)
    n = C.c_int32(0)
    c = loc.to_c()
    rc = _L().o3s_localizability_remap(C.byref(c), int(min_category), P.ctypes.data_as(dp), Q.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(n))
    if rc != _lib.OK:
        raise ValueError(f"[{rc}] o3s_localizability_remap refused its arguments")
    return out.reshape(4, 4).T.copy(), int(n.value)


def minimize_degeneracy(icp, reading_xyz, ids, dists2, weights, dset: DegeneracySet, values=None):
    """o3s_icp_minimize_degeneracy: ICP.minimize with the step constrained to have no component along the directions of `dset`
    -> (T 4x4, A' 6x6, b', x): the constrained system as the solver took it.  values = (rot_values, trans_values): the step's
    components along the directions instead of zero (o3s_icp_minimize_degeneracy_values)."""
    return icp.minimize_degeneracy(reading_xyz, ids, dists2, weights, dset, values=values)


def partial_estimate(icp, reading_c, reference_c, normals, params: LocalizabilityParams):
    """o3s_degeneracy_partial_estimate: the analysis and the strong-pair sums of (K, 3) arrays of ALREADY centred pairs
    -> (Localizability, DegeneracyPartial); the first is o3s_localizability_estimate's result bit for bit."""
    fp = C.POINTER(C.c_float)
    p = np.ascontiguousarray(reading_c, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(reference_c, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if not (p.shape == q.shape == n.shape):
        raise ValueError("reading_c, reference_c and normals must have the same shape (K, 3)")
    L = _bind(icp._L)
    lc, pc, out = LocalizabilityC(), params.to_c(), DegeneracyPartialC()
    icp._check(L.o3s_degen_partial_estimate(icp._h, p.ctypes.data_as(fp), q.ctypes.data_as(fp), n.ctypes.data_as(fp), p.shape[0], C.byref(pc),
                                            C.byref(lc), C.byref(out)))
    return Localizability.from_c(lc), DegeneracyPartial.from_c(out)
