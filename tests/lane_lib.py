"""ctypes wrappers of the lane-local pins (tests/lane_cases).  TEST INFRASTRUCTURE ONLY: the cases of lane_cases.h compiled three times
-- for the host emulator (g++ -DDIAL_EMU -ffp-contract=off), and for gfx950 with the product flags and with the IEEE flags of
dial_mpc_amd/_lib.py (hipcc cross-compiles without a GPU).  Same staleness check and atomic rename as tests/prim_lib.py.  Nothing under
dial_mpc_amd/ loads these libraries.  One lane runs one case: inputs are float32 / int32 rows, results uint32 rows (raw bits)."""
import ctypes
import os
import subprocess

import numpy as np

from dial_mpc_amd import _abi, _lib

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lane_cases")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dial_mpc_amd", "csrc")

S_POINT, S_SEGSEG, S_FRAME = range(3)
K_FKEY, K_PACK, K_OPEN, K_UPDATE, K_LAZY, K_GATE, K_RESULT = range(7)
SENTINEL = 0x7FC5A5A5     # what a result word holds before a case runs (a NaN no case produces)


def _stale(so, main):
    srcs = [os.path.join(_HERE, main), os.path.join(_HERE, "lane_cases.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")] + [_abi.HEADER]
    return not (os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(f) for f in srcs))


def _compile(so, cmd):
    tmp = f"{so}.{os.getpid()}.tmp"     # atomic: parallel test workers may all find the library stale at once
    try:
        subprocess.check_call(cmd + ["-o", tmp])
        os.replace(tmp, so)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return so


def build_emu(defines=(), tag="", csrc=_CSRC):
    """defines / tag / csrc: a VARIANT next to the default library (a one-change build of the code under test)."""
    so = os.path.join(_HERE, f"liblanes_emu{tag}.so")
    if not tag and not _stale(so, "lanes_emu.cpp"):
        return so
    return _compile(so, ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-ffp-contract=off", *defines,
                         "-I", csrc, "-I", _HERE, os.path.join(_HERE, "lanes_emu.cpp")])


def build_dev(ieee, defines=(), tag="", csrc=_CSRC):
    """The device library with the product flags (-DDIAL_FUSED_DPP, contraction, fast math) or with the IEEE flags."""
    so = os.path.join(_HERE, f"liblanes_{'ieee' if ieee else 'fast'}{tag}.so")
    if not tag and not _stale(so, "lanes.hip"):
        return so
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _lib._COMMON + (_lib._IEEE if ieee else _lib._FAST)
    return _compile(so, [hipcc, *flags, *defines, "-shared", "-I", csrc, "-I", _HERE, os.path.join(_HERE, "lanes.hip")])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sizes(lib):
    v = (ctypes.c_int * 12)()
    lib.lane_sizes(v)
    return list(v)


class _Side:
    def _init_sizes(self):
        (self.G_IN, self.G_OUT, self.S_IN, self.S_OUT, self.K_IN, self.K_OUT, self.U_IN, self.U_OUT, self.T_IN, self.T_OUT,
         self.POLY_WORDS, self.POLY_STRIDE) = _sizes(self.lib)

    @staticmethod
    def _rows(x, width, dtype):
        """[n, <= width] -> contiguous [n, width] of dtype, bits preserved, missing columns 0."""
        x = np.asarray(x)
        assert x.ndim == 2 and x.shape[1] <= width and x.dtype.itemsize == 4, (x.shape, x.dtype, width)
        r = np.zeros((len(x), width), dtype)
        r.view(np.uint32)[:, :x.shape[1]] = np.ascontiguousarray(x).view(np.uint32)
        return r

    def geom(self, rows, fill=0):
        """rows [n, 22] float32 (kind, sub, g1[10], g2[10]; g = pos[3], quat[4], size[3]) -> [n, 13] uint32 (dist, pos[3], frame[9])."""
        return self._run("lane_geom", self._rows(rows, self.G_IN, np.float32), self.G_OUT, int(fill))

    def seg(self, rows):
        return self._run("lane_seg", self._rows(rows, self.S_IN, np.float32), self.S_OUT)

    def key(self, op, rows, par=0):
        return self._run("lane_key", self._rows(rows, self.K_IN, np.int32), self.K_OUT, int(op), int(par))

    def key_uniform(self, rows, rule, minmax):
        return self._run("lane_key_uniform", self._rows(rows, self.U_IN, np.int32), self.U_OUT, int(rule), int(bool(minmax)))

    def trig(self, rows):
        return self._run("lane_trig", self._rows(rows, self.T_IN, np.float32), self.T_OUT)


class Emu(_Side):
    def __init__(self, defines=(), tag="", csrc=_CSRC):
        self.lib = ctypes.CDLL(build_emu(defines, tag, csrc))
        self._init_sizes()

    def _run(self, fn, x, nout, *args):
        out = np.full((len(x), nout), SENTINEL, np.uint32)
        assert getattr(self.lib, fn)(_p(x), _p(out), len(x), *args) == 0, fn
        return out


class Dev(_Side):
    """The device side: the same calls on torch allocations, launched on the current stream."""

    def __init__(self, ieee, defines=(), tag="", csrc=_CSRC):
        import torch
        self.torch = torch
        self.ieee = ieee
        self.lib = ctypes.CDLL(build_dev(ieee, defines, tag, csrc))
        self._init_sizes()

    def _run(self, fn, x, nout, *args):
        t = self.torch
        xin = t.from_numpy(x.view(np.int32)).cuda()      # raw bits: NaN payloads survive
        out = t.full((len(x), nout), SENTINEL, dtype=t.int32, device="cuda")
        rc = getattr(self.lib, fn)(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), len(x), *args,
                                   ctypes.c_void_p(t.cuda.current_stream().cuda_stream))
        assert rc == 0, f"{fn}: HIP error {rc}"
        t.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)
