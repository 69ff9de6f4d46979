"""Synthetic blocks on both sides of the plan compiler's and the launchers' shape guards.

Every case is a tiny ONNX graph (tests/onnx_build.py) together with the same computation written
directly in torch.float64 on CPU tensors (torch.nn.functional, pads applied with F.pad): the
reference shares no parsing, pad or layout logic with the code under test.  A case names the guard
it sits on and the side, the plan steps zr_plan_describe must show (plan_tokens), and a regular
expression one profiled kernel name must match (want) and / or none may match (forbid).

Families: A depthwise -> 1x1 (launch_dwpw), B expand -> depthwise -> project (launch_ir), C the
low-resolution inverted residual (launch_irl), D the bottleneck (launch_bneck), E the GEMM family
(choose_gemm), F the remaining steps, G output placement (NCHW, NHWC, offset inside a Concat).
The generic forms come first in every family.

Block inputs are internal (CNHW) tensors: a "feeder" 1x1 conv of the 3-channel graph input makes
them, as a stem does in the shipped models.  Seeds come from the case name.  Weights and inputs are
uniform(-1, 1), 1x1 / dense weights scaled by 1 / sqrt(K); every conv has a bias, PRelu slopes are
per channel unless a case says otherwise.

Two sides the issue lists cannot be reached from a valid graph and have no case: a shortcut with
more channels than its conv (Add needs equal shapes and Pad only grows, so lower_add's r_C > M test
never fires), and the launchers' pointer-alignment tests on arena tensors and weights (the arena
and the weight blocks are 16-byte aligned by construction); the output-alignment test of the GEMM
vector store is reached through a Concat offset (E/heads_misaligned).
"""
from __future__ import annotations

import math
import re
import zlib
from dataclasses import dataclass
from functools import cached_property
from typing import Callable, Optional, Sequence

import numpy as np

import onnx_build as ob
from zaru_amd import _lib as _zaru_lib

# torch's wheel bundles a ROCm runtime of its own, and whichever HIP runtime a process loads first
# serves every library in it: load the project's library (and with it the runtime it links) before
# torch, so the code under test runs on its own runtime wherever this module is imported first
_zaru_lib.lib()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

F64 = torch.float64
KINDS = ("gemm", "dw", "direct", "elt", "resize", "gap", "dwpw", "dwgap", "gdc")
NHWC_ERROR = "NHWC output on a non-GEMM step"


def plan_tokens(txt: str):
    """One token per plan step: kind [stem] /resN /ir /grpN (N != 1) /nhwc (position stride != 1)."""
    out = []
    for line in txt.splitlines():
        if line.split(" ")[0] not in KINDS:
            continue
        f = dict(p.split("=", 1) for p in line.split(" ") if "=" in p)
        t = line.split(" in=")[0]
        if f["res"] != "0":
            t += "/res" + f["res"]
        if f["ir"] != "0":
            t += "/ir"
        if f["grp"] != "1":
            t += "/grp" + f["grp"]
        if f["oP"] not in ("0", "1"):
            t += "/nhwc"
        out.append(t)
    return out


class Graph:
    """ONNX nodes and their float64 torch restatement, built side by side."""

    def __init__(self, name: str, in_shape):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.in_shape = tuple(in_shape)
        self.nodes, self.inits, self.ops = [], {}, []
        self.shape = {"x": (1,) + self.in_shape}
        self._n = 0

    def _name(self, p):
        self._n += 1
        return f"{p}{self._n}"

    def _init(self, a, p="w"):
        n = self._name(p)
        self.inits[n] = a
        return n

    def uniform(self, shape, scale=1.0):
        return (self.rng.uniform(-1.0, 1.0, size=shape) * scale).astype(np.float32)

    def _emit(self, op, ins, fn, tins, **attrs):
        y = self._name(op.lower())
        self.nodes.append(ob.node(op, ins, [y], **attrs))
        self.ops.append((y, fn, tuple(tins)))
        self.shape[y] = tuple(fn(*[torch.zeros(self.shape[t], dtype=F64) for t in tins]).shape)
        return y

    # ---- operators
    def conv(self, x, cout, k, s=1, pads=0, group=1):
        kh, kw = (k, k) if isinstance(k, int) else k
        pt, pl, pb, pr = (pads,) * 4 if isinstance(pads, int) else pads
        cg = self.shape[x][1] // group
        w = self.uniform((cout, cg, kh, kw), 1.0 / math.sqrt(cg * kh * kw) if group == 1 else 1.0)
        b = self.uniform((cout,))
        wt, bt = torch.from_numpy(w).double(), torch.from_numpy(b).double()

        def fn(t):
            return F.conv2d(F.pad(t, (pl, pr, pt, pb)), wt, bt, stride=s, groups=group)
        return self._emit("Conv", [x, self._init(w), self._init(b, "b")], fn, [x], kernel_shape=[kh, kw],
                          strides=[s, s], pads=[pt, pl, pb, pr], group=group)

    def dw(self, x, k, s, pad):
        return self.conv(x, self.shape[x][1], k, s, PADS[pad](k, s), group=self.shape[x][1])

    def relu(self, x):
        return self._emit("Relu", [x], torch.relu, [x])

    def sigmoid(self, x):
        return self._emit("Sigmoid", [x], torch.sigmoid, [x])

    def clip(self, x, lo=0.0, hi=6.0):
        ins = [x, self._init(np.array(lo, np.float32), "c"), self._init(np.array(hi, np.float32), "c")]
        return self._emit("Clip", ins, lambda t: t.clamp(lo, hi), [x])

    def prelu(self, x, single=False):
        c = self.shape[x][1]
        sl = self.uniform((1,) if single else (c, 1, 1))
        st = torch.from_numpy(sl).double().reshape(1, -1, 1, 1)
        return self._emit("PRelu", [x, self._init(sl, "s")], lambda t: torch.where(t < 0, t * st, t), [x])

    def act(self, x, kind):
        if not kind:
            return x
        return {"relu": self.relu, "clip": self.clip, "prelu": self.prelu, "sigmoid": self.sigmoid,
                "prelu1": lambda v: self.prelu(v, single=True)}[kind](x)

    def add(self, a, b):
        return self._emit("Add", [a, b], lambda u, v: u + v, [a, b])

    def maxpool(self, x):
        return self._emit("MaxPool", [x], lambda t: F.max_pool2d(t, 2, 2), [x], kernel_shape=[2, 2], strides=[2, 2])

    def padc(self, x, cout):
        extra = cout - self.shape[x][1]
        pads = self._init(np.array([0, 0, 0, 0, 0, extra, 0, 0], np.int64), "p")
        return self._emit("Pad", [x, pads], lambda t: F.pad(t, (0, 0, 0, 0, 0, extra)), [x], mode="constant")

    def resize(self, x, oh, ow):
        sizes = self._init(np.array([1, self.shape[x][1], oh, ow], np.int64), "z")

        def fn(t):
            return F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False)
        return self._emit("Resize", [x, "", "", sizes], fn, [x], mode="linear",
                          coordinate_transformation_mode="half_pixel")

    def gap(self, x, spelling="global"):
        h, w = self.shape[x][2:]
        if spelling == "global":
            return self._emit("GlobalAveragePool", [x], lambda t: t.mean((2, 3), keepdim=True), [x])
        if spelling == "avgpool":
            return self._emit("AveragePool", [x], lambda t: t.mean((2, 3), keepdim=True), [x], kernel_shape=[h, w])
        if spelling == "mean23":
            return self._emit("ReduceMean", [x], lambda t: t.mean((2, 3), keepdim=True), [x], axes=[2, 3], keepdims=1)
        m = self._emit("ReduceMean", [x], lambda t: t.mean(3), [x], axes=[3], keepdims=0)  # over W, then H
        return self._emit("ReduceMean", [m], lambda t: t.mean(2), [m], axes=[2], keepdims=0)

    def gemm(self, x, m, trans_b, alpha, beta):
        k = self.shape[x][1]
        b = self.uniform((m, k) if trans_b else (k, m), 1.0 / math.sqrt(k))
        c = self.uniform((m,))
        bt, ct = torch.from_numpy(b).double(), torch.from_numpy(c).double()
        return self._emit("Gemm", [x, self._init(b), self._init(c, "b")],
                          lambda t: alpha * (t @ (bt.T if trans_b else bt)) + beta * ct, [x],
                          transB=int(trans_b), alpha=float(alpha), beta=float(beta))

    def reshape(self, x, dims):
        return self._emit("Reshape", [x, self._init(np.array(dims, np.int64), "r")],
                          lambda t: t.reshape((t.shape[0],) + tuple(dims[1:])), [x])

    def transpose(self, x):
        return self._emit("Transpose", [x], lambda t: t.permute(0, 2, 3, 1), [x], perm=[0, 2, 3, 1])

    def concat(self, xs):
        return self._emit("Concat", list(xs), lambda *t: torch.cat(t, 1), xs, axis=1)

    def feeder(self, c):
        """The block input as an internal tensor: a 1x1 conv of the graph input."""
        return self.conv("x", c, 1)

    # ---- results
    def onnx(self, outs):
        return ob.model(self.nodes, {"x": [1, *self.in_shape]}, {o: list(self.shape[o]) for o in outs}, self.inits)

    def run(self, x, outs):
        env = {"x": torch.from_numpy(np.asarray(x)).double()}
        for y, fn, tins in self.ops:
            env[y] = fn(*[env[t] for t in tins])
        return [env[o].contiguous().numpy() for o in outs]


def _tf(k, s):  # TF-style 'same': [top, left, bottom, right]
    return (k // 2,) * 4 if s == 1 else (k // 2 - 1, k // 2 - 1, k // 2, k // 2)


PADS = {"tf": _tf, "sym": lambda k, s: (k // 2,) * 4, "none": lambda k, s: (0, 0, 0, 0)}


@dataclass
class Case:
    name: str
    in_shape: tuple
    build: Callable[[Graph], Sequence[str]]  # adds the nodes, returns the graph outputs
    batches: tuple = (1, 3)
    kinds: Optional[Sequence[str]] = None    # plan_tokens the compiled plan must show
    want: Optional[str] = None               # a profiled kernel name must match (re.match)
    forbid: Optional[str] = None             # no profiled kernel name may match
    error: Optional[str] = None              # compile_plan must refuse the graph with this message

    @cached_property
    def _built(self):
        g = Graph(self.name, self.in_shape)
        return g, list(self.build(g))

    @property
    def onnx(self) -> bytes:
        g, outs = self._built
        return g.onnx(outs)

    def ref(self, x):
        g, outs = self._built
        return g.run(x, outs)

    def input(self, batch: int):
        rng = np.random.default_rng(zlib.crc32(f"{self.name}/{batch}".encode()))
        return rng.uniform(-1.0, 1.0, size=(batch, *self.in_shape)).astype(np.float32)


def input_alone(case: Case, batch: int, image: int):
    return case.input(batch)[image:image + 1]


# ---------------------------------------------------------------- output placement (family G)
def place(g: Graph, y, how):
    """y as a graph output: plain NCHW, NHWC through a folded Transpose, or behind a second head
    inside a Concat (cat: both transposed, as the SSD heads; catc: channel-major)."""
    if how == "nchw":
        return [y]
    if how == "nhwc":
        return [g.transpose(y)]
    h = g.conv("x", 4, 1)  # reads the graph input: never a launch-group partner of the block's steps
    if how == "cat":
        h, y = g.transpose(h), g.transpose(y)
    return [g.concat([g.reshape(h, [1, -1, 1]), g.reshape(y, [1, -1, 1])])]


def placed(kinds, how, step=-1):
    k = list(kinds)
    if how in ("nhwc", "cat"):
        k[step] += "/nhwc"
    if how in ("cat", "catc"):
        k.append("gemm/nhwc" if how == "cat" else "gemm")
    return k


def shortcut(g, t0, cout, short):
    if not short:
        return None
    r = g.maxpool(t0) if short.startswith("pool") else t0
    return g.padc(r, cout) if short.endswith("pad") or short == "padc" else r


RES = {None: 0, "id": 1, "padc": 1, "pool": 2, "poolpad": 2}
CASES: list[Case] = []


def case(name, in_shape, build, **kw):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, tuple(in_shape), build, **kw))


# ---------------------------------------------------------------- A: depthwise -> 1x1
def dwpw(k, s, pad, hw, cin, cout, short=None, act=None, dwclip=False, how="nchw", flip=False):
    def build(g):
        t0 = g.feeder(cin)
        d = g.dw(t0, k, s, pad)
        if dwclip:
            d = g.clip(d)
        y = g.conv(d, cout, 1)
        r = shortcut(g, t0, cout, short)
        if r:
            y = g.add(r, y) if flip else g.add(y, r)
        return place(g, g.act(y, act), how)
    res = RES[short]
    return build, placed(["gemm", "dwpw" + (f"/res{res}" if res else "")], how)


def A(note, k, s, pad, hw, cin, cout, short, act, dwclip=False, batches=(1, 3), want=None, forbid=None, **kw):
    name = f"A/{note}/k{k}s{s}{pad}_{hw[0]}x{hw[1]}_{cin}to{cout}_{short or 'plain'}" + ("_dwclip" if dwclip else "")
    build, kinds = dwpw(k, s, pad, hw, cin, cout, short, act, dwclip, **kw)
    case(name, (3, *hw), build, batches=batches, kinds=kinds, want=want, forbid=forbid)


# the register-staged MFMA form first (K % 4 != 0 keeps LDS-DMA off), then LDS-DMA, then VALU
A("K%4!=0,no_v4", 3, 1, "tf", (9, 13), 17, 17, "id", "prelu", want=r"dwpw_kernel<.*false>")
A("K%4!=0,v4", 3, 1, "tf", (8, 8), 17, 32, "padc", "relu", batches=(1, 3, 37), want=r"dwpw_kernel<.*true>")
A("K%4!=0,nopad", 5, 1, "none", (9, 13), 17, 8, None, "prelu", want=r"dwpw_kernel<.*false>")
A("dma_runs_exceed_lds", 5, 2, "tf", (16, 128), 8, 49, None, "relu", want=r"dwpw_kernel<")
A("dma_runs_fit_lds", 5, 2, "tf", (16, 64), 8, 49, None, "relu", want=r"dwpw_dma")
A("M>48", 3, 1, "tf", (16, 16), 24, 49, None, "relu", want=r"dwpw_dma", forbid=r"dwpw_v")
A("K*M>2048", 3, 1, "tf", (16, 16), 96, 32, None, None, want=r"dwpw_dma", forbid=r"dwpw_v")
A("W%4!=0,P>=256", 3, 1, "tf", (18, 15), 8, 8, "id", "relu", want=r"dwpw_dma", forbid=r"dwpw_v")
A("P<256,W%4==0", 3, 1, "tf", (20, 12), 8, 8, "id", "prelu", want=r"dwpw_dma", forbid=r"dwpw_v")
A("P<256,W%4!=0", 5, 1, "tf", (16, 15), 8, 8, "id", "relu", want=r"dwpw_dma", forbid=r"dwpw_v")
A("W>248", 3, 1, "tf", (4, 252), 8, 8, "id", "relu", want=r"dwpw_(dma|kernel)", forbid=r"dwpw_v")
A("valu_rows_exceed_lds", 5, 2, "tf", (8, 248), 8, 8, None, "relu", want=r"dwpw_(dma|kernel)", forbid=r"dwpw_v")
A("mfma,Mpad96", 5, 1, "tf", (6, 6), 96, 96, "id", "relu", batches=(1, 3, 37), want=r"dwpw_dma")
A("mfma,Mpad256", 3, 1, "tf", (3, 3), 256, 256, "id", "prelu", want=r"dwpw_dma")
A("mfma,Mpad256,pool", 5, 2, "tf", (6, 6), 96, 256, "poolpad", "relu", want=r"dwpw_dma")
A("mfma,2x2", 3, 1, "tf", (2, 2), 24, 40, "padc", "relu", batches=(1, 3, 37), want=r"dwpw_dma")
A("mfma,Mpad32", 3, 2, "tf", (16, 16), 256, 8, None, "relu", want=r"dwpw_dma")
A("mfma,flipped_add", 3, 1, "tf", (6, 6), 24, 24, "id", "relu", want=r"dwpw_dma", flip=True)
A("sym_pads:no_row_tasks", 3, 2, "sym", (12, 12), 24, 48, "poolpad", "prelu", want=r"dwpw_dma_kernel<.*,0>")
# (48 outputs: Mpad 64 takes 64-column tiles, whose stride-2 input runs fit the DMA buffers at every
# batch; with Mpad 32 the 128-column tiles span whole images and the step is register-staged)
A("odd_side:W!=OW*S", 3, 2, "tf", (15, 15), 24, 48, "poolpad", "relu", want=r"dwpw_dma_kernel<.*,0>")
A("odd_side:W!=OW*S,P=256", 3, 2, "tf", (33, 33), 8, 48, "poolpad", "relu", want=r"dwpw_dma_kernel<.*,0>")
A("odd_side,128_column_tiles:runs_exceed_lds", 3, 2, "tf", (33, 33), 8, 16, "poolpad", "relu", want=r"dwpw_kernel<")
A("tf_pads:row_tasks", 3, 2, "tf", (12, 12), 24, 48, "poolpad", "prelu", want=r"dwpw_dma(_pin)?_kernel<.*,[248]>")
A("nopad,s2", 5, 2, "none", (20, 12), 8, 48, None, "relu", want=r"dwpw_dma_kernel<.*,0>")
A("valu,P=256,vres", 3, 1, "tf", (16, 16), 8, 8, "id", "relu", batches=(1, 3, 37), want=r"dwpw_vres_kernel<3,1,16,")
A("valu,rC<M,vres", 3, 1, "tf", (16, 16), 8, 16, "padc", "prelu", want=r"dwpw_vres_kernel<3,1,16,")
A("valu,K%4!=0", 3, 1, "tf", (16, 16), 17, 16, None, "prelu", want=r"dwpw_valu_kernel<3,1,16,")
A("valu,M=17:CO32", 3, 1, "tf", (16, 16), 24, 17, None, "relu", want=r"dwpw_valu_kernel<3,1,32,")
A("valu,M=32,vres", 3, 1, "tf", (16, 16), 24, 32, "padc", "prelu", batches=(1, 37), want=r"dwpw_vres_kernel<3,1,32,")
A("valu,M=40:CO48,s1_single_buffer", 5, 1, "tf", (16, 16), 24, 40, None, "relu", dwclip=True,
  want=r"dwpw_valu_kernel<5,1,48,false")
A("valu,M=48,vres", 3, 1, "tf", (16, 16), 24, 48, "padc", "relu", want=r"dwpw_vres_kernel<3,1,48,")
A("valu,M=48,dw_act:no_vres", 3, 1, "tf", (16, 16), 24, 48, "padc", "relu", dwclip=True,
  want=r"dwpw_valu_kernel<3,1,48,false")
A("valu,s2,pool_vres", 3, 2, "tf", (32, 32), 8, 16, "poolpad", "prelu", want=r"dwpw_vres_kernel<3,2,16,")
A("valu,k5s2,pool_vres", 5, 2, "tf", (32, 32), 24, 32, "poolpad", "relu", want=r"dwpw_vres_kernel<5,2,32,")
A("valu,sym_pads:no_vres", 3, 2, "sym", (32, 32), 8, 16, "poolpad", "relu", want=r"dwpw_valu_kernel<3,2,16,true")
A("valu,M=48,s2_double_buffer", 5, 2, "tf", (32, 32), 24, 48, None, "relu", dwclip=True,
  want=r"dwpw_valu_kernel<5,2,48,true")
A("valu,nopad", 3, 1, "none", (18, 20), 8, 8, None, "relu", want=r"dwpw_valu_kernel<3,1,16,")
A("valu,W=248", 3, 1, "tf", (4, 248), 8, 8, "id", "relu", want=r"dwpw_vres_kernel<3,1,16,")


def _dwpw_siblings(g):  # two blocks over one tensor, as FaceMesh's mesh / flag branches: one grid
    # (Mpad 32: the one layout without stacked M tiles, which the grouped kernel needs, at any batch)
    t0 = g.feeder(32)
    return [g.relu(g.add(g.conv(g.dw(t0, 3, 1, "tf"), 32, 1), t0)), g.prelu(g.conv(g.dw(t0, 3, 1, "tf"), 24, 1))]


case("A/siblings_one_launch/k3s1tf_6x6_32to32+24", (3, 6, 6), _dwpw_siblings,
     kinds=["gemm", "dwpw/res1/grp2", "dwpw/grp0"], want=r"dwpw_dma_group_kernel<3,1,")


def _dwpw_shared(g):  # the 1x1's output has a second reader: the Add cannot fold into its epilogue
    t0 = g.feeder(24)
    y = g.conv(g.dw(t0, 3, 1, "tf"), 24, 1)
    return [g.relu(g.add(y, t0)), g.gap(y)]


case("A/shared_conv:unfused_add/k3s1tf_6x6_24to24", (3, 6, 6), _dwpw_shared,
     kinds=["gemm", "dwpw", "elt", "gap"], want=r"elt_kernel")


# ---------------------------------------------------------------- B / C / D: expand -> dw -> project
def ir_block(k, s, pad, cin, cexp, cout, short, eact="clip", dact="clip", act=None, how="nchw", reader2=False,
             tail=False):
    def build(g):
        t0 = g.feeder(cin)
        e = g.act(g.conv(t0, cexp, 1), eact)
        d = g.act(g.dw(e, k, s, pad), dact)
        y = g.conv(d, cout, 1)
        r = shortcut(g, t0, cout, short)
        if r:
            y = g.add(y, r)
        y = g.act(y, act)
        if tail:  # the block's output stays internal: a 1x1 conv behind it writes the graph output
            y = g.conv(y, 5, 1)
        outs = place(g, y, how)
        return outs + ([g.gap(e)] if reader2 else [])
    res = RES[short]
    kinds = ["gemm", "gemm" if reader2 else "gemm/ir", "dwpw" + (f"/res{res}" if res else "")]
    kinds = placed(kinds + (["gemm"] if tail else []), how)
    return build, kinds + (["gap"] if reader2 else [])


def IR(fam, note, k, s, pad, hw, cin, cexp, cout, short, batches=(1, 3), want=None, forbid=None, **kw):
    name = f"{fam}/{note}/k{k}s{s}{pad}_{hw[0]}x{hw[1]}_{cin}-{cexp}-{cout}_{short or 'plain'}"
    build, kinds = ir_block(k, s, pad, cin, cexp, cout, short, **kw)
    case(name, (3, *hw), build, batches=batches, kinds=kinds, want=want, forbid=forbid)


# near misses (unfused: the generic launches) first
IR("B", "Cin24:unfused", 3, 1, "tf", (16, 32), 24, 64, 24, "id", forbid=r"ir_kernel")
IR("B", "Cexp40:unfused", 3, 1, "tf", (16, 32), 16, 40, 16, "id", forbid=r"ir_kernel")
IR("B", "Cout40:unfused", 3, 1, "tf", (16, 32), 16, 64, 40, "padc", forbid=r"ir_kernel")
IR("B", "sym_pads_s2:unfused", 3, 2, "sym", (40, 48), 16, 64, 24, "poolpad", forbid=r"ir_kernel")
IR("B", "odd_side:W!=OW*S:unfused", 3, 2, "tf", (17, 33), 16, 64, 24, None, forbid=r"ir_kernel")
IR("B", "k5s1:unfused", 5, 1, "tf", (16, 32), 16, 64, 16, "id", forbid=r"ir_kernel")
IR("B", "prelu_expand:unfused", 3, 1, "tf", (16, 32), 16, 64, 16, "id", eact="prelu", forbid=r"ir_kernel")
IR("B", "expanded_read_twice:unmarked", 3, 1, "tf", (16, 32), 16, 64, 16, "id", reader2=True, forbid=r"ir_kernel")
# the round-6 hole: a pooled shortcut at 5x5 s2 (pad 1) must not take the fused kernel
IR("B", "k5s2_pooled:unfused", 5, 2, "tf", (40, 48), 16, 64, 16, "pool", forbid=r"ir_kernel")
IR("B", "k5s2_pooled_padded:unfused", 5, 2, "tf", (16, 32), 16, 64, 24, "poolpad", forbid=r"ir_kernel")
IR("B", "whole_tiles", 3, 1, "tf", (16, 32), 16, 64, 16, "id", want=r"ir_kernel<3,1,16>")
IR("B", "partial_tiles", 3, 1, "tf", (20, 40), 16, 64, 24, None, want=r"ir_kernel<3,1,32>")
IR("B", "partial_tiles,relu", 3, 1, "tf", (20, 40), 16, 64, 16, "id", eact="relu", dact="relu", act="relu",
   want=r"ir_kernel<3,1,16>")
IR("B", "s2_pooled_padded", 3, 2, "tf", (40, 48), 16, 64, 24, "poolpad", want=r"ir_kernel<3,2,32>")
IR("B", "s2_pooled", 3, 2, "tf", (16, 32), 16, 64, 16, "pool", want=r"ir_kernel<3,2,16>")
IR("B", "s2_partial_tiles", 3, 2, "tf", (20, 40), 16, 64, 24, None, want=r"ir_kernel<3,2,32>")
IR("B", "k5s2", 5, 2, "tf", (40, 48), 16, 64, 24, None, want=r"ir_kernel<5,2,32>")
IR("B", "k5s2_partial_tiles", 5, 2, "tf", (20, 40), 16, 64, 16, None, want=r"ir_kernel<5,2,16>")

IR("C", "13x13:unfused", 3, 1, "tf", (13, 13), 48, 96, 48, "id", forbid=r"irl_kernel")
IR("C", "Cexp48:unfused", 3, 1, "tf", (14, 14), 48, 48, 48, "id", forbid=r"irl_kernel")
IR("C", "sigmoid_expand:unfused", 3, 1, "tf", (14, 14), 48, 96, 48, "id", eact="sigmoid", forbid=r"irl_kernel")
IR("C", "s2_pooled:unfused", 5, 2, "tf", (14, 14), 64, 96, 112, "poolpad", forbid=r"irl_kernel")
for _short in ("id", None):
    IR("C", "14_cx48_k3", 3, 1, "tf", (14, 14), 48, 96, 48 if _short else 64, _short, want=r"irl_kernel<3,14,1,48,2>")
    IR("C", "14_cx48_k5", 5, 1, "tf", (14, 14), 48, 96, 48 if _short else 40, _short, want=r"irl_kernel<5,14,1,48,2>")
    IR("C", "14_cx64_k5", 5, 1, "tf", (14, 14), 64, 96, 64, _short, want=r"irl_kernel<5,14,1,64,2>")
    IR("C", "7_cx112_k5", 5, 1, "tf", (7, 7), 112, 96, 112, _short, want=r"irl_kernel<5,7,1,112,4>")
IR("C", "14to7_cx64_k5s2", 5, 2, "tf", (14, 14), 64, 96, 112, None, want=r"irl_kernel<5,14,2,64,4>")
# 257 images: odd and above the CU count, two images per workgroup with the last slot empty
IR("C", "7_cx112_k5,257_images", 5, 1, "tf", (7, 7), 112, 64, 112, "id", batches=(257,),
   want=r"irl_kernel<5,7,1,112,4,2>")
IR("C", "14to7_cx64_k5s2,257_images", 5, 2, "tf", (14, 14), 64, 64, 112, None, batches=(257,),
   want=r"irl_kernel<5,14,2,64,4,2>")

# (the fused kernel writes a plain CNHW tensor: the block output is internal, as in FaceMesh V2)
_BN = dict(eact="prelu", dact=None, act="prelu", tail=True)
IR("D", "C64_32x32:unfused", 3, 1, "tf", (32, 32), 64, 32, 64, "id", batches=(2, 3), forbid=r"bneck_kernel", **_BN)
IR("D", "no_shortcut:unfused", 3, 1, "tf", (64, 64), 32, 16, 32, None, batches=(2, 3), forbid=r"bneck_kernel", **_BN)
IR("D", "k5:unfused", 5, 1, "tf", (64, 64), 32, 16, 32, "id", batches=(2, 3), forbid=r"bneck_kernel", **_BN)
IR("D", "C16_128x128", 3, 1, "tf", (128, 128), 16, 8, 16, "id", batches=(2, 3), want=r"bneck_kernel<16,128>", **_BN)
IR("D", "C32_64x64", 3, 1, "tf", (64, 64), 32, 16, 32, "id", batches=(2, 3), want=r"bneck_kernel<32,64>", **_BN)


# ---------------------------------------------------------------- E: the GEMM family
def gemm_1x1(K, M, variant):
    def build(g):
        y = g.conv(g.feeder(K), M, 1)
        if variant == "add":
            return [g.prelu(g.add(g.relu(y), g.conv("x", M, 1)))]
        return place(g, g.relu(y) if M % 2 and M > 1 else y, "nhwc" if variant == "nhwc" else "nchw")
    if variant == "add":  # the shortcut's conv comes after in ONNX order: the fused step moves behind it
        return build, ["gemm", "gemm", "gemm/res1"]
    # (M = 1: NHWC and NCHW are the same layout, the position stride stays 1)
    return build, placed(["gemm", "gemm"], "nhwc" if variant == "nhwc" and M > 1 else "nchw")


# (K, M, plane side, batches, kernel): ncols % 4 != 0 with one M tile and K <= 128 takes the small-K
# form, everything else on a CNHW tensor the LDS-tiled one (whole float4 tails inside the arena row)
for _K, _M, _hw, _b, _kern in ((3, 1, 1, (1, 3, 5), r"gemm_smallk_kernel<1>"),
                               (16, 31, 3, (1, 3, 5), r"gemm_smallk_kernel<1>"),
                               (64, 32, 7, (1, 3, 5), r"gemm_smallk_kernel<2>"),
                               (65, 32, 3, (1, 3, 5), r"gemm_smallk_kernel<3>"),
                               (130, 32, 7, (1, 3, 5), r"gemm_tiled_kernel<1,1,"),
                               (16, 33, 7, (1, 3, 5), r"gemm_tiled_kernel<1,1,"),
                               (256, 100, 3, (1, 3, 5), r"gemm_tiled_kernel<1,1,"),
                               (64, 100, 8, (1, 5), r"gemm_tiled_kernel<1,1,"),
                               (256, 1, 8, (1, 3), r"gemm_tiled_kernel<1,1,")):
    for _v in ("plain", "add", "nhwc"):
        _build, _kinds = gemm_1x1(_K, _M, _v)
        case(f"E/1x1_K{_K}_M{_M}_P{_hw * _hw}_{_v}", (3, _hw, _hw), _build, batches=_b, kinds=_kinds, want=_kern)

case("E/1x1_on_graph_input:generic", (130, 3, 3), lambda g: [g.conv("x", 33, 1)], batches=(1, 3, 5),
     kinds=["gemm"], want=r"gemm_kernel<\d,false>")


def full_plane(C, kh, kw, M, add=False):
    def build(g):
        y = g.conv(g.feeder(C), M, (kh, kw))
        return [g.add(y, g.conv(g.gap("x"), M, 1)) if add else y]
    return build


case("E/full_plane_square_4_chunks", (3, 4, 4), full_plane(8, 4, 4, 20), batches=(1, 3, 17),
     kinds=["gemm", "gemm"], want=r"gemm_rows_kernel<true, 0>")
case("E/full_plane_nonsquare", (3, 3, 5), full_plane(7, 3, 5, 33), batches=(1, 3, 17),
     kinds=["gemm", "gemm"], want=r"gemm_rows_kernel<true, 0>")
case("E/full_plane_9_chunks", (3, 4, 4), full_plane(18, 4, 4, 40), batches=(1, 3, 17),
     kinds=["gemm", "gemm"], want=r"gemm_rows_kernel<true, 9>")
case("E/full_plane_residual:generic", (3, 3, 5), full_plane(7, 3, 5, 33, add=True), batches=(1, 3),
     kinds=["gemm", "gap", "gemm", "gemm/res1"], want=r"gemm_kernel<\d,true>")
for _k in (2, 4):
    case(f"E/patch_{_k}x{_k}s{_k}", (3, 8, 8), lambda g, k=_k: [g.prelu(g.conv(g.feeder(8), 24, k, k))],
         kinds=["gemm", "gemm"], want=r"gemm_kernel<\d,true>")
for _tb in (0, 1):
    case(f"E/Gemm_transB{_tb}_alpha_beta", (3, 1, 1),
         lambda g, tb=_tb: [g.gemm(g.reshape(g.relu(g.feeder(40)), [1, 40]), 10, tb, 0.75, 1.5)],
         batches=(1, 3, 5), kinds=["gemm", "gemm"], want=r"gemm_")


def ssd_heads(first_anchors):
    """BlazeFace's heads: classifier / regressor pairs over two scales, transposed, reshaped and
    concatenated into one score and one box output (group launches, output offsets)."""
    def build(g):
        t0 = g.feeder(16)
        t1 = g.conv(g.dw(t0, 3, 2, "tf"), 24, 1)
        cls, reg = [], []
        for t, a in ((t0, first_anchors), (t1, 6)):
            cls.append(g.reshape(g.transpose(g.conv(t, a, 1)), [1, -1, 1]))
            reg.append(g.reshape(g.transpose(g.conv(t, a * 16, 1)), [1, -1, 16]))
        return [g.concat(cls), g.concat(reg)]
    return build


_HEADS = ["gemm", "dwpw", "gemm/grp2/nhwc", "gemm/grp0/nhwc", "gemm/grp2/nhwc", "gemm/grp0/nhwc"]
case("E/heads_grouped", (3, 8, 8), ssd_heads(2), batches=(1, 3), kinds=_HEADS, want=r"gemm_\w*group_kernel")
# 3 anchors on 7^2: the second scale's scores start 147 floats into the output (not 16-byte aligned)
case("E/heads_misaligned", (3, 7, 7), ssd_heads(3), batches=(1, 3), kinds=_HEADS, want=r"gemm_")


# ---------------------------------------------------------------- F: the remaining steps
def dw_alone(k, s, pad, readers):
    def build(g):
        d = g.relu(g.dw(g.feeder(12), k, s, pad))
        return [d] if readers == 0 else [g.conv(d, 8, 1), g.prelu(g.conv(d, 40, 1))]
    return build


for _k, _s, _pad, _hw in ((3, 1, "tf", (3, 3)), (5, 2, "tf", (3, 3)), (3, 1, "tf", (33, 32)), (5, 1, "sym", (33, 32)),
                          (3, 2, "tf", (33, 32)), (5, 2, "none", (33, 32))):
    case(f"F/dw_output/k{_k}s{_s}{_pad}_{_hw[0]}x{_hw[1]}", (3, *_hw), dw_alone(_k, _s, _pad, 0),
         kinds=["gemm", "dw"], want=rf"dw_kernel<{_k},{_s}>")
case("F/dw_two_readers/k3s1tf_33x32", (3, 33, 32), dw_alone(3, 1, "tf", 2),
     kinds=["gemm", "dw", "gemm/grp2", "gemm/grp0"], want=r"dw_kernel<3,1>")
case("F/dw_two_readers/k5s2tf_3x3", (3, 3, 3), dw_alone(5, 2, "tf", 2), batches=(1, 3, 5),
     kinds=["gemm", "dw", "gemm/grp2", "gemm/grp0"], want=r"dw_kernel<5,2>")

for _k, _s, _pad, _hw, _co, _act in ((3, 1, "tf", (9, 35), 1, "relu"), (3, 2, "tf", (17, 19), 7, "prelu"),
                                     (3, 2, "sym", (16, 64), 16, "relu"), (3, 1, "tf", (8, 33), 24, "prelu"),
                                     (3, 2, "tf", (17, 19), 64, "relu"), (5, 1, "tf", (9, 35), 7, "prelu"),
                                     (5, 2, "tf", (17, 19), 24, "relu"), (5, 2, "sym", (17, 19), 32, "prelu"),
                                     (5, 1, "none", (12, 37), 16, "clip")):
    case(f"F/stem/k{_k}s{_s}{_pad}_{_hw[0]}x{_hw[1]}_3to{_co}", (3, *_hw),
         lambda g, k=_k, s=_s, pad=_pad, co=_co, act=_act: [g.act(g.conv("x", co, k, s, PADS[pad](k, s)), act)],
         kinds=["direct stem"], want=rf"stem_kernel<{_k},{_s},{16 if _co <= 16 else 24 if _co <= 24 else 32 if _co <= 32 else 64},false>")
case("F/stem_Cout65:direct", (3, 9, 35), lambda g: [g.relu(g.conv("x", 65, 3, 1, 1))], kinds=["direct"],
     want=r"direct_kernel", forbid=r"stem_kernel")
case("F/stem_k5_Cout33:direct", (3, 9, 35), lambda g: [g.relu(g.conv("x", 33, 5, 1, 2))], kinds=["direct"],
     want=r"direct_kernel", forbid=r"stem_kernel")
for _ci, _k, _s, _co, _hw in ((4, 3, 1, 5, (9, 35)), (3, 7, 2, 9, (17, 19)), (40, 3, 2, 9, (17, 67)), (37, 3, 2, 5, (17, 67))):
    # Cin 40 / 37 at stride 2: the LDS chunk halves to 10 channels, which does not divide 37
    case(f"F/direct/k{_k}s{_s}_{_hw[0]}x{_hw[1]}_{_ci}to{_co}", (_ci, *_hw),
         lambda g, k=_k, s=_s, co=_co: [g.prelu(g.conv("x", co, k, s, k // 2))], kinds=["direct"], want=r"direct_kernel")

# (both scales are exact in f32, so the kernel's f32 sample positions are the reference's)
for _ih, _iw, _oh, _ow in ((6, 5, 12, 8), (5, 6, 8, 12)):
    case(f"F/resize_{_ih}x{_iw}_to_{_oh}x{_ow}", (3, _ih, _iw), lambda g, oh=_oh, ow=_ow: [g.resize(g.feeder(5), oh, ow)],
         kinds=["gemm", "resize"], want=r"resize_kernel")


def _fpn(g):  # BlazeFace full range: conv(12^2) + Resize(6^2 branch), the conv first in ONNX order
    t0 = g.feeder(8)
    lat = g.conv(t0, 8, 1)
    up = g.resize(g.conv(g.dw(t0, 3, 2, "tf"), 8, 1), 12, 12)
    return [g.relu(g.add(lat, up))]


case("F/resize_shortcut_after_its_conv", (3, 12, 12), _fpn, kinds=["gemm", "dwpw", "resize", "gemm/res1"],
     want=r"resize_kernel")
for _sp in ("global", "avgpool", "mean23", "mean3_mean2"):
    case(f"F/gap_{_sp}", (3, 5, 7), lambda g, sp=_sp: [g.gap(g.feeder(19), sp)], kinds=["gemm", "gap"],
         want=r"gap_kernel")
case("F/dw_gap_16x32:fused", (3, 16, 32), lambda g: [g.gap(g.relu(g.dw(g.feeder(12), 3, 1, "tf")))],
     kinds=["gemm", "dwgap"], want=r"dwgap_kernel")
case("F/dw_gap_16x33:two_launches", (3, 16, 33), lambda g: [g.gap(g.relu(g.dw(g.feeder(12), 5, 1, "tf")))],
     kinds=["gemm", "dw", "gap"], forbid=r"dwgap_kernel")
case("F/dw_gap_k5s2_9x11:fused", (3, 9, 11), lambda g: [g.gap(g.clip(g.dw(g.feeder(12), 5, 2, "tf")))],
     kinds=["gemm", "dwgap"], want=r"dwgap_kernel")
case("F/whole_plane_depthwise_7x7", (3, 7, 7), lambda g: [g.prelu(g.conv(g.feeder(20), 20, 7, group=20))],
     batches=(1, 3, 5), kinds=["gemm", "gdc"], want=r"gdc_kernel")
case("F/maxpool_pad_materialised", (3, 6, 10), lambda g: [g.conv(g.padc(g.maxpool(g.feeder(5)), 8), 6, 1)],
     kinds=["gemm", "elt", "elt", "gemm"], want=r"elt_kernel")


def _shared(g):  # both Add operands have a second reader; the Sigmoid's input too
    a, b = g.feeder(6), g.feeder(6)
    return [g.add(a, b), g.sigmoid(a), g.relu(b)]


case("F/add_of_shared_values+sigmoid_of_shared", (3, 5, 7), _shared, kinds=["gemm", "gemm", "elt", "elt", "elt"],
     want=r"elt_kernel")
case("F/prelu_single_slope", (3, 5, 7), lambda g: [g.act(g.conv(g.feeder(9), 11, 1), "prelu1")],
     kinds=["gemm", "gemm"], want=r"gemm_")


def _vector_concat(g):  # the 68-point nets: pooled features of two scales concatenated, then dense
    t0 = g.feeder(10)
    t1 = g.relu(g.conv(g.dw(t0, 3, 2, "tf"), 14, 1))
    return [g.conv(g.concat([g.gap(t0), g.gap(t1)]), 7, 1)]


case("F/internal_vector_concat", (3, 6, 6), _vector_concat, kinds=["gemm", "dwpw", "gap", "gap", "gemm"],
     want=r"gap_kernel")


# ---------------------------------------------------------------- G: output placement
def G_dwpw(how):
    return dwpw(3, 1, "tf", (6, 10), 20, 24, "padc", "prelu", how=how)


def G_valu(how):
    return dwpw(3, 1, "tf", (16, 16), 8, 8, "id", "relu", how=how)


for _how in ("nhwc", "cat", "catc"):
    _b, _k = G_dwpw(_how)
    case(f"G/dwpw_mfma_{_how}", (3, 6, 10), _b, kinds=_k, want=r"dwpw_dma")
    _b, _k = G_valu(_how)
    case(f"G/dwpw_valu_{_how}", (3, 16, 16), _b, kinds=_k, want=r"dwpw_v")
    case(f"G/gemm_{_how}", (3, 7, 7), lambda g, how=_how: place(g, g.conv(g.feeder(16), 33, 1), how),
         batches=(1, 3, 4), kinds=placed(["gemm", "gemm"], _how), want=r"gemm_")
# the fused blocks write plain NCHW only: behind a Transpose the pair runs unfused
for _how in ("nhwc", "cat"):
    _b, _k = ir_block(3, 1, "tf", 16, 64, 16, "id", how=_how)
    case(f"G/ir_{_how}:unfused", (3, 16, 32), _b, kinds=_k, forbid=r"ir_kernel")
    _b, _k = ir_block(5, 1, "tf", 112, 96, 112, "id", how=_how)
    case(f"G/irl_{_how}:unfused", (3, 7, 7), _b, kinds=_k, forbid=r"irl_kernel")
_b, _k = ir_block(3, 1, "tf", 32, 16, 32, "id", **dict(_BN, tail=False))
case("G/bneck_graph_output:unfused", (3, 64, 64), _b, batches=(2,), kinds=_k, forbid=r"bneck_kernel")
_b, _k = ir_block(3, 1, "tf", 16, 64, 16, "id", how="catc")
case("G/ir_catc", (3, 16, 32), _b, kinds=_k, want=r"ir_kernel<3,1,16>")

# Steps other than gemm / dwpw carry no position stride: NHWC on them over more than one position is
# refused by compile_plan (NHWC_ERROR); a channel-major Concat offset (catc) is fine
_NON_GEMM = {
    "dw": ((3, 5, 7), lambda g: g.relu(g.dw(g.feeder(6), 3, 1, "tf")), ["gemm", "dw"]),
    "stem": ((3, 9, 11), lambda g: g.relu(g.conv("x", 8, 3, 2, _tf(3, 2))), ["direct stem"]),
    "direct": ((4, 5, 7), lambda g: g.relu(g.conv("x", 5, 3, 1, 1)), ["direct"]),
    "elt_add": ((3, 5, 7), lambda g: (lambda a: g.add(g.relu(a), g.sigmoid(a)))(g.feeder(6)), ["gemm", "elt", "elt", "elt"]),
    "resize": ((3, 5, 6), lambda g: g.resize(g.feeder(5), 8, 12), ["gemm", "resize"]),
}
for _n, (_shape, _fn, _k) in _NON_GEMM.items():
    case(f"G/{_n}_catc", _shape, lambda g, fn=_fn: place(g, fn(g), "catc"), kinds=placed(_k, "catc"))
    for _how in ("nhwc", "cat") if _n == "dw" else ("nhwc",):
        case(f"G/{_n}_{_how}:refused", _shape, lambda g, fn=_fn, how=_how: place(g, fn(g), how), error=NHWC_ERROR)
# one position per image: NHWC and NCHW coincide, any step may sit behind the Transpose
_VECTORS = {
    "gap": ((3, 5, 7), lambda g: g.gap(g.feeder(19)), ["gemm", "gap"]),
    "dwgap": ((3, 8, 8), lambda g: g.gap(g.relu(g.dw(g.feeder(12), 3, 1, "tf"))), ["gemm", "dwgap"]),
    "gdc": ((3, 7, 7), lambda g: g.conv(g.feeder(20), 20, 7, group=20), ["gemm", "gdc"]),
}
for _n, (_shape, _fn, _k) in _VECTORS.items():
    for _how in ("nhwc", "cat", "catc") if _n == "gap" else ("nhwc",):
        case(f"G/{_n}_{_how}", _shape, lambda g, fn=_fn, how=_how: place(g, fn(g), how), kinds=placed(_k, _how))

BY_NAME = {c.name: c for c in CASES}


def profile_kernels(txt: str):
    """Kernel names of a zr_profile_read text (a name may hold a space: 'gemm_rows_kernel<true, 9>')."""
    return [l.rsplit(None, 4)[0] for l in txt.splitlines() if l.strip()]


def kernels_ok(c: Case, kernels):
    if c.want and not any(re.match(c.want, k) for k in kernels):
        return f"no kernel matches {c.want!r}: {kernels}"
    if c.forbid and any(re.match(c.forbid, k) for k in kernels):
        return f"a kernel matches {c.forbid!r}: {kernels}"
    return None


def run_case(c: Case):
    """The case on the GPU through the public API: {batch: (outputs, profiled kernel names)} for
    every batch of the case, plus "alone": image 1 of the batch-3 input run by itself.  None when
    compile_plan refuses the graph with the case's error."""
    import ctypes as C

    from zaru_amd._lib import ZaruError, check, lib
    from zaru_amd.nn import NeuralNetwork
    try:
        net = NeuralNetwork.from_onnx(c.onnx).load()
    except ZaruError as e:
        if c.error and c.error in str(e):
            return None
        raise
    check(lib().zr_profile_enable(net._h, 1))
    buf, need = C.create_string_buffer(1 << 16), C.c_size_t()
    res = {}
    for b in c.batches + (("alone",) if 3 in c.batches else ()):
        outs = net.estimate(c.input(3)[1:2] if b == "alone" else c.input(b))
        check(lib().zr_profile_read(net._h, buf, len(buf), C.byref(need)))  # (returns and clears)
        res[b] = (outs, profile_kernels(buf.value.decode()))
    return res
