"""Synthetic stem -> first BlazeBlock graphs on both sides of the fused stem + block launch's guards
(form "stemblock": plan.cpp mark_stem_blocks, kernels/stemblock.hip), built with the synth_models
builders: the ONNX graph and its torch.float64 restatement side by side.

FUSED: the pair must run as one stem_dwpw_kernel launch.  GUARDS: the pair must run as the two
launches it always did (no stem_dwpw_kernel in the profile).  The cases are registered under
synth_models.BY_NAME (not CASES: the synth table's own tests stay as they are) so that
test_gpu_synth's reference cache finds them by name.

One guard has no case: a stem output that is also a graph output.  compile_plan refuses every graph
whose output is consumed internally ("graph output ... is also consumed internally"), so such a
stem never reaches mark_stem_blocks; its test of the output's kind is kept as a defence.
"""
import synth_models as S

SYMBOL = r"stem_dwpw_kernel<"


def stem_block(k, cs, sact, cout, short, act, spad="tf", sstride=2, bk=3, bstride=1, dwclip=False, reader2=False):
    def build(g):
        s = g.act(g.conv("x", cs, k, sstride, S.PADS[spad](k, sstride)), sact)
        d = g.dw(s, bk, bstride, "tf")
        if dwclip:
            d = g.clip(d)
        y = g.conv(d, cout, 1)
        r = S.shortcut(g, s, cout, short)
        if r:
            y = g.add(y, r)
        outs = [g.act(y, act)]
        if reader2:
            outs.append(g.gap(s))
        return outs
    res = S.RES[short]
    return build, ["direct stem", "dwpw" + (f"/res{res}" if res else "")] + (["gap"] if reader2 else [])


def _case(table, name, in_hw, want=None, forbid=None, **kw):
    build, kinds = stem_block(**kw)
    c = S.Case(name, (3, *in_hw), build, batches=(1, 3), kinds=kinds, want=want, forbid=forbid)
    assert name not in S.BY_NAME, name
    S.BY_NAME[name] = c
    table.append(c)


FUSED: list = []
# 20x36 stem plane: partial tiles in both directions, W % 4 == 0, P >= 256
_case(FUSED, "SB/k3_16to16_prelu_40x72", (40, 72), want=r"stem_dwpw_kernel<3,2,16,16,false>",
      k=3, cs=16, sact="prelu", cout=16, short="id", act="prelu")
# 17x40: odd height, channel-padded shortcut (r_C 24 < M 28), the 32-output instance
_case(FUSED, "SB/k5_24to28_relu_34x80", (34, 80), want=r"stem_dwpw_kernel<5,2,24,32,false>",
      k=5, cs=24, sact="relu", cout=28, short="padc", act="relu")
# 16x32: all four plane edges inside one tile column
_case(FUSED, "SB/k3_16to16_relu_32x64", (32, 64), want=r"stem_dwpw_kernel<3,2,16,16,false>",
      k=3, cs=16, sact="relu", cout=16, short="id", act="relu")
# symmetric stem pads (pad 1 on every side), 19x36: odd height, the last tile row 3 rows high
_case(FUSED, "SB/k3_sym_pads_16to16_37x71", (37, 71), want=r"stem_dwpw_kernel<3,2,16,16,false>",
      k=3, cs=16, sact="prelu", cout=16, short="id", act="relu", spad="sym")

GUARDS: list = []
_K3 = dict(k=3, cs=16, sact="prelu", cout=16, short="id", act="prelu")
_K5 = dict(k=5, cs=24, sact="relu", cout=28, short="padc", act="relu")
_case(GUARDS, "SB/guard/stem_read_twice", (40, 72), forbid=SYMBOL, **dict(_K3, reader2=True))
_case(GUARDS, "SB/guard/stem_Cout40", (40, 72), forbid=SYMBOL, **dict(_K3, cs=40, cout=40))
_case(GUARDS, "SB/guard/block_s2_pooled", (40, 72), forbid=SYMBOL, **dict(_K3, bstride=2, short="pool"))
_case(GUARDS, "SB/guard/block_s2_pooled_padded", (34, 80), forbid=SYMBOL, **dict(_K5, bstride=2, short="poolpad"))
_case(GUARDS, "SB/guard/no_shortcut", (40, 72), forbid=SYMBOL, **dict(_K3, short=None))
_case(GUARDS, "SB/guard/dw_clip", (40, 72), forbid=SYMBOL, **dict(_K3, dwclip=True))
_case(GUARDS, "SB/guard/W18:W%4!=0", (40, 36), forbid=SYMBOL, **_K3)
_case(GUARDS, "SB/guard/12x20:P<256", (24, 40), forbid=SYMBOL, **_K5)
# shapes without an instance of the fused kernel
_case(GUARDS, "SB/guard/stem_s1", (20, 36), forbid=SYMBOL, **dict(_K3, sstride=1))
_case(GUARDS, "SB/guard/block_k5", (34, 80), forbid=SYMBOL, **dict(_K5, bk=5))
_case(GUARDS, "SB/guard/stem_k3_to24", (40, 72), forbid=SYMBOL, **dict(_K5, k=3))
_case(GUARDS, "SB/guard/stem_k5_to16", (40, 72), forbid=SYMBOL, **dict(_K3, k=5))
_case(GUARDS, "SB/guard/stem16_block24", (40, 72), forbid=SYMBOL, **dict(_K3, cout=24, short="padc"))
_case(GUARDS, "SB/guard/stem_32", (40, 72), forbid=SYMBOL, **dict(_K3, cs=32, cout=32))

ALL = FUSED + GUARDS
