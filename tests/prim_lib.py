"""ctypes wrappers of the wave.h / register L D L^T pins (tests/wave_prims).  TEST INFRASTRUCTURE ONLY: the cases of prim_cases.h and
chol_cases.h compiled three times -- for the host emulator (g++ -DDIAL_EMU), and for gfx950 with the product flags and with the IEEE
flags of dial_mpc_amd/_lib.py (hipcc cross-compiles without a GPU).  Same staleness check and atomic rename as tests/emu_lib.py.
Nothing under dial_mpc_amd/ loads these libraries."""
import ctypes
import os
import subprocess

import numpy as np

from dial_mpc_amd import _abi, _lib

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_prims")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dial_mpc_amd", "csrc")
_HEADERS = ["prim_cases.h", "chol_cases.h"]

C_ROW, C_PICK, C_BCAST, C_PERM, C_MASK, C_COMPACT, C_VSUMS, C_FSUMS, C_CONTRACT, C_FMA, C_FNMA, C_MUL, C_RCP = range(13)
# name -> (inst of chol_run, N, dof tree: PARENTS key or None = dense).  The last four are the generic path's DimsPadV<N> (rollout_body.h)
INST = {"go2": (0, 18, "go2"), "h1": (1, 25, "h1"), "h1loco": (2, 17, "h1loco"), "allegro": (3, 22, "allegro"),
        "allegro_dense": (4, 22, None), "crate_climb": (5, 18, "go2"), "push_crate": (6, 26, "push_crate"),
        "push_crate_dense": (7, 26, None), "capacity_dense": (8, 28, None)}
# the dof trees of dial_mpc_amd/csrc/cmodel.h (TopoGo2, TopoH1, TopoH1Loco, TopoAllegro, TopoH1PushCrate)
_H1 = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 5, 11, 12, 13, 14, 5, 16, 17, 18, 19, 16, 21, 22, 23]
PARENTS = {"go2": [-1, 0, 1, 2, 3, 4, 5, 6, 7, 5, 9, 10, 5, 12, 13, 5, 15, 16],
           "h1": _H1, "push_crate": _H1 + [-1],
           "h1loco": [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 5, 11, 12, 13, 14, 5],
           "allegro": [-1, 0, 1, 2, 3, 4, -1, 6, 7, 8, -1, 10, 11, 12, -1, 14, 15, 16, -1, 18, 19, 20]}

def _stale(so, main):
    srcs = [os.path.join(_HERE, main)] + [os.path.join(_HERE, h) for h in _HEADERS]
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


def build_emu():
    so = os.path.join(_HERE, "libprims_emu.so")
    if not _stale(so, "prims_emu.cpp"):
        return so
    return _compile(so, ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-ffp-contract=off",
                         "-I", _CSRC, os.path.join(_HERE, "prims_emu.cpp")])


def build_dev(ieee):
    """The device library with the product flags (-DDIAL_FUSED_DPP, contraction, fast math) or with the IEEE flags."""
    so = os.path.join(_HERE, f"libprims_{'ieee' if ieee else 'fast'}.so")
    if not _stale(so, "prims.hip"):
        return so
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _lib._COMMON + (_lib._IEEE if ieee else _lib._FAST)
    return _compile(so, [hipcc, *flags, "-shared", "-I", _CSRC, os.path.join(_HERE, "prims.hip")])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sizes(lib):
    v = [ctypes.c_int() for _ in range(5)]
    lib.prim_sizes(*[ctypes.byref(x) for x in v])
    return [x.value for x in v]


SENTINEL = 0x7FC5A5A5     # what a result word holds before a case runs (a NaN no case produces)


class Emu:
    """The host side.  Inputs [nset, NIN, 64] float32, results [nset, NOUT, 64] uint32 (raw bits)."""

    def __init__(self):
        self.lib = ctypes.CDLL(build_emu())
        self.NIN, self.NOUT, self.NCASE, self.CH_A, self.CH_OUT = _sizes(self.lib)
        for f in (self.lib.prim_row_tree, self.lib.prim_tree64, self.lib.prim_tree32):
            f.restype = ctypes.c_float

    def pack(self, *inputs):
        """[nset, 64] arrays -> the [nset, NIN, 64] input block (unused inputs are 0)."""
        x = np.zeros((len(inputs[0]), self.NIN, 64), np.float32)
        for k, a in enumerate(inputs):
            x.view(np.uint32)[:, k, :] = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return x

    def wave(self, case, x, par=0):
        out = np.full((len(x), self.NOUT, 64), SENTINEL, np.uint32)
        assert self.lib.prim_run_wave(_p(x), _p(out), len(x), case, par) == 0
        return out

    def half(self, case, x, par=0, halves=(0, 1)):
        """Both halves' data through the one-half emulator, into one result block laid out like the device's."""
        out = np.full((len(x), self.NOUT, 64), SENTINEL, np.uint32)
        for h in halves:
            assert self.lib.prim_run_half(_p(x), _p(out), len(x), case, par, h) == 0
        return out

    def chol(self, name, form, A, b, scr0=None, alias=0):
        """A [nsys, N, N] float32 (exact zeros off the pattern), b [nsys, N] -> dict of x, dinv (by dof), x_reuse, scratch [nsys, N, S]."""
        args, N, S = _chol_args(self, name, form, A, b, scr0)
        out = np.zeros((len(A), self.CH_OUT), np.uint32)
        assert self.lib.chol_run(INST[name][0], form, *[_p(a) for a in args], _p(out), len(A), alias) == 0
        return _chol_unpack(out, N, S, form)

    def row_tree(self, v):
        return np.float32(self.lib.prim_row_tree(_p(np.ascontiguousarray(v, np.float32))))

    def tree64(self, v):
        return np.float32(self.lib.prim_tree64(_p(np.ascontiguousarray(v, np.float32))))

    def tree32(self, v):
        return np.float32(self.lib.prim_tree32(_p(np.ascontiguousarray(v, np.float32))))

    def fmaf(self, a, b, c):
        a, b, c = (np.ascontiguousarray(np.broadcast_to(t, np.broadcast(a, b, c).shape), np.float32) for t in (a, b, c))
        out = np.empty_like(a)
        self.lib.prim_fmaf(a.size, _p(a), _p(b), _p(c), _p(out))
        return out

    def mulf(self, a, b):
        a, b = (np.ascontiguousarray(np.broadcast_to(t, np.broadcast(a, b).shape), np.float32) for t in (a, b))
        out = np.empty_like(a)
        self.lib.prim_mulf(a.size, _p(a), _p(b), _p(out))
        return out


def _chol_args(sizes, name, form, A, b, scr0):
    N = INST[name][1]
    S = (N + 3) & ~3
    nsys = len(A)
    Ap = np.zeros((nsys, sizes.CH_A), np.float32)
    sq = np.zeros((nsys, N, S), np.float32)
    sq[:, :, :N] = A
    Ap[:, :N * S] = sq.reshape(nsys, -1)
    bp = np.full((nsys, 64), np.nan, np.float32)      # lanes >= N of the right-hand side register: NaN the result must not see
    for k in range(nsys):
        off = 32 * (k & 1) if form == 2 else 0
        bp[k, off:off + N] = b[k]
    sp = np.zeros((nsys, sizes.CH_A), np.float32)
    if scr0 is not None:
        sp[:, :N * S] = np.asarray(scr0, np.float32).reshape(nsys, -1)
    return (Ap, bp, sp), N, S


def _chol_unpack(out, N, S, form):
    nsys = len(out)
    f = out.view(np.float32)
    lanes = f[:, :192].reshape(nsys, 3, 64)
    off = np.array([32 * (k & 1) if form == 2 else 0 for k in range(nsys)])
    take = lambda slot: np.stack([lanes[k, slot, off[k]:off[k] + N] for k in range(nsys)])
    return dict(x=take(0), dinv=take(1)[:, ::-1].copy(), x_reuse=take(2), scratch=f[:, 192:192 + N * S].reshape(nsys, N, S).copy())


class Dev:
    """The device side: the same calls on torch allocations, launched on the current stream."""

    def __init__(self, ieee):
        import torch
        self.torch = torch
        self.ieee = ieee
        self.lib = ctypes.CDLL(build_dev(ieee))
        self.NIN, self.NOUT, self.NCASE, self.CH_A, self.CH_OUT = _sizes(self.lib)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()      # raw bits: NaN payloads survive

    def _blank(self, n):
        return self.torch.full((n, self.NOUT, 64), SENTINEL, dtype=self.torch.int32, device="cuda")

    def _down(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)

    def wave(self, case, x, par=0):
        xin, out = self._up(x), self._blank(len(x))
        rc = self.lib.prim_run_wave(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), len(x), case, par, self._stream())
        assert rc == 0, f"prim_run_wave: HIP error {rc}"
        return self._down(out)

    def half(self, case, x, par=0, mode=0, case1=0, par1=0):
        xin, out = self._up(x), self._blank(len(x))
        rc = self.lib.prim_run_half(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), len(x), case, par, case1, par1,
                                    mode, self._stream())
        assert rc == 0, f"prim_run_half: HIP error {rc}"
        return self._down(out)

    def chol(self, name, form, A, b, scr0=None, alias=0):
        args, N, S = _chol_args(self, name, form, A, b, scr0)
        dev = [self._up(a) for a in args]
        out = self.torch.zeros((len(A), self.CH_OUT), dtype=self.torch.int32, device="cuda")
        rc = self.lib.chol_run(INST[name][0], form, *[ctypes.c_void_p(t.data_ptr()) for t in dev], ctypes.c_void_p(out.data_ptr()),
                               len(A), alias, self._stream())
        assert rc == 0, f"chol_run: HIP error {rc}"
        return _chol_unpack(self._down(out), N, S, form)
