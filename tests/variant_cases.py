"""The kernel variants the training step selects at the product shape, as a table (test infrastructure; a plain module).

The dispatchers of csrc/conv.hip, wgrad.hip, conv_x6.hip, wino.hip and wino4.hip choose a kernel template instance per launch shape, so steps of
m = 2..8 clips run different instances and epilogues.  A CLASS is what one matrix launch exercises:

  conv / bf16-split conv:  (variant string of pc_conv_variant, epilogue flags, activation, activation from a channel on, batch groups > 1,
                            per-group weights, channel-slice input, channel-slice output)
  Winograd:                (variant string of pc_wino_variant, epilogue flags, activation, channel-slice input, channel-slice output,
                            temporal map (ta, tc, tden), KT, Ti != T)
  weight gradient:         (variant string of pc_wgrad_variant with the slice count folded to k1 / kN, batched problems, sub-lattice D,
                            channel-slice D, channel-slice S, trimmed taps)

CASES holds one entry per class that occurs in the plans for n = 2..8, UCF-101 and JHMDB, 224 x 224, four lanes: the launch with the
least work at the smallest n where the class occurs, as the descriptor the plan carries.  tests/test_variant_coverage_cpu.py checks that the
table is complete, consistent and free of dead entries; tests/test_variants_gpu.py runs every entry against float64.

Regenerate after a dispatcher change:  python -m tests.variant_cases > tests/variant_cases_table.py
"""
import re

from picons_amd import capi, desc as D, step as pstep
from picons_amd.plan import Plan, _cdesc, _wdesc

SIZES = range(2, 9)
DATASETS = ("ucf101", "jhmdb")
EPI_FLAGS = capi.F_ACCUM | capi.F_BIAS | capi.F_CSCALE | capi.F_BNPART | capi.F_NFAST | capi.F_TOUT
WGRAD_VEC3 = ("istr", "ntap", "ioff0", "istep", "wk0", "doff")
WINO_FIELDS = [f for f, _t in capi.WinoDesc._fields_]


def unflatten_wgrad(flat):
    d, q = {}, 0
    for f in D.WGRAD_FIELDS:
        if f in WGRAD_VEC3:
            d[f] = [int(x) for x in flat[q:q + 3]]
            q += 3
        else:
            d[f] = int(flat[q])
            q += 1
    assert q == len(flat)
    return d


def wino_struct(ints):
    st = capi.WinoDesc()
    for f, v in zip(WINO_FIELDS, ints):
        setattr(st, f, int(v))
    return st


def conv_class(d, ws_floats):
    """d: conv descriptor dict as the op carries it; ws_floats: the tail-split workspace the op brings (OP_CONV_X6), else 0."""
    v = capi.variant("pc_conv_variant", _cdesc(d), int(ws_floats))
    return ("conv", v, d["flags"] & EPI_FLAGS, d["act"], d["act_c0"] > 0, d["groups"] > 1, d["wgstride"] != 0, d["ldi"] != d["Ci"], d["ldo"] != d["Co"])


def wino_class(ints):
    import ctypes as C
    st = wino_struct(ints)
    v = capi.variant("pc_wino_variant", C.byref(st), None)
    return ("wino", v, st.flags & EPI_FLAGS, st.act, st.ldi != st.Ci, st.ldo != st.Co, (st.ta, st.tc, st.tden), st.KT, st.Ti != st.T)


def wgrad_class(d):
    v = capi.variant("pc_wgrad_variant", _wdesc(d))
    v = re.sub(r":k(\d+):", lambda m: ":k1:" if m.group(1) == "1" else ":kN:", v)
    trimmed = [d["ntap"][0] != d["KT"], d["ntap"][1] != d["KH"], d["ntap"][2] != d["KW"]]
    return ("wgrad", v, d["nbatch"] > 1, d["Td"] > 0, d["ldd"] != d["Cd"], d["lds"] != d["Cs"], any(trimmed))


def build_plan(n, dataset):
    jh = dataset == "jhmdb"
    p = Plan(21 if jh else 24, 224, n=n, groups=2, training=True, jhmdb=jh, lanes=4, early_adam=True)
    p.build_forward(); p.build_loss(pstep.default_args(bv=True, n_frames=5, wt_cons=0.1)); p.build_backward(); p.build_adam(); p.finalize()
    return p


def _work(kind, d):
    if kind == "conv":
        return d["N"] * d["Tq"] * d["Hq"] * d["Wq"] * d["Co"] * d["Ci"] * d["ntap"][0] * d["ntap"][1] * d["ntap"][2]
    if kind == "wgrad":
        return d["N"] * d["Tq"] * d["Hq"] * d["Wq"] * d["Cd"] * d["Cs"] * d["ntap"][0] * d["ntap"][1] * d["ntap"][2] * max(1, d["nbatch"])
    return d[0] * d[1] * d[2] * d[3] * d[4] * d[6] * d[8]


def plan_launches(p):
    """Every matrix launch of a finalized plan -> (class, kind, flat descriptor ints, tail-split workspace floats, list name)."""
    for name in p.lists:
        for op in p.lists[name]:
            kind, ints = op[0], [int(x) for x in op[1]]
            if kind in (capi.OP_CONV, capi.OP_CONV_X6):
                ws = int(op[4][1]) if kind == capi.OP_CONV_X6 else 0
                yield conv_class(D.unflatten_conv(ints), ws), "conv", ints, ws, name
            elif kind == capi.OP_WINO_CONV:
                yield wino_class(ints), "wino", ints, 0, name
            elif kind == capi.OP_WGRAD:
                yield wgrad_class(unflatten_wgrad(ints)), "wgrad", ints, 0, name
            elif kind == capi.OP_WGRAD_MULTI:
                for d, _p in p.wjobs[op[3][0][1]]:          # p = [("WJOBS", index into Plan.wjobs)]
                    flat = D.flatten(d, D.WGRAD_FIELDS)
                    yield wgrad_class(unflatten_wgrad(flat)), "wgrad", flat, 0, name


def case_class(case):
    kind, ints, ws = case["kind"], case["desc"], case["ws"]
    if kind == "conv":
        return conv_class(D.unflatten_conv(ints), ws)
    if kind == "wino":
        return wino_class(ints)
    return wgrad_class(unflatten_wgrad(ints))


def walk():
    """-> {class: dict(sizes={(dataset, n)}, best=(n, work, dataset, kind, ints, ws, list))} over every plan of SIZES x DATASETS."""
    seen = {}
    for ds in DATASETS:
        for n in SIZES:
            for cls, kind, ints, ws, name in plan_launches(build_plan(n, ds)):
                e = seen.setdefault(cls, dict(sizes=set(), best=None))
                e["sizes"].add((ds, n))
                d = ints if kind == "wino" else (D.unflatten_conv(ints) if kind == "conv" else unflatten_wgrad(ints))
                key = (n, _work(kind, d), DATASETS.index(ds))
                if e["best"] is None or key < e["best"][0]:
                    e["best"] = (key, dict(kind=kind, n=n, dataset=ds, list=name, ws=ws, desc=ints))
    return seen


def case_id(case):
    return "%s-%s" % (case["name"], re.sub(r"[^A-Za-z0-9_]+", "_", case["cls"][1]).strip("_"))


try:
    from tests.variant_cases_table import CASES
except ImportError:          # first generation
    CASES = []


if __name__ == "__main__":
    seen = walk()
    print('"""Generated by `python -m tests.variant_cases` (tests/variant_cases.py explains the fields): one launch per kernel-variant class of the\n'
          'training step at 224 x 224, n = 2..8 clips.  `sizes`: the n at which the class occurs (u = UCF-101, j = JHMDB)."""')
    print("CASES = [")
    for q, cls in enumerate(sorted(seen, key=repr)):
        c = seen[cls]["best"][1]
        sizes = ",".join("%s%d" % (ds[0], n) for ds, n in sorted(seen[cls]["sizes"]))
        print("    dict(name=%r, kind=%r, n=%d, dataset=%r, list=%r, ws=%d, sizes=%r,\n         cls=%r,\n         desc=%r)," %
              ("c%03d" % q, c["kind"], c["n"], c["dataset"], c["list"], c["ws"], sizes, cls, c["desc"]))
    print("]")
