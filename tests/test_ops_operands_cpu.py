"""CPU: what every wrapper of the eval/detect half of ops checks on its operands, without a GPU.  One row per wrapper: a set of good operands
made of small CPU tensors (F = 2, H = 4, W = 8, S = 4, one clip, one view, K = 2, L = 1, P = A = 1, two threshold words) and one-operand
perturbations of it.  ops.ptr raises RuntimeError("... no CPU fallback") for a tensor that is not on a GPU before anything reaches the library,
so every case ends on the host in one of two ways: "V", the wrapper's own ValueError naming the wrapper, or "R", that RuntimeError -- every
check took the operands.  The letters were recorded from the code as it stood before the wrappers were given shared operand checks: the
table pins that the shared checks accept and refuse what the open-coded ones did.  "-": not a case (the operand cannot be perturbed that
way, or the open-coded check let it escape: a non-tensor as AttributeError / TypeError, flat logits as IndexError).  Run as a program
(with the repository root on the path) the file prints the table as the code at hand behaves, for new rows.  The decode_* functions:
numpy in, torch in, same arrays out."""
import inspect
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from picons_amd import capi, ops

F, H, W, S, K, L, P, A = 2, 4, 8, 4, 2, 1, 1, 1
WORDS = [100, 200]
VIEWS, STARTS = [(0, 0, 0)], [0]
OTHER = {torch.uint8: torch.int32, torch.float32: torch.float64, torch.int32: torch.float32, torch.int16: torch.int32}
# the perturbations of one tensor operand, in the order of a row's letters
PERTURB = ("dtype", "strided", "fewer", "more", "meta", "numpy")


def u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def i16(*shape):
    return torch.zeros(*shape, dtype=torch.int16)


def perturbed(t, how):
    """The operand t, wrong in one way; None where it cannot be."""
    if how == "dtype":
        return t.to(OTHER[t.dtype])
    if how == "strided":                     # the same shape and element count, every other element of a wider tensor
        return None if t.numel() < 2 else t.new_zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],))[..., ::2]
    if how == "fewer":
        return None if t.numel() < 1 else t.new_zeros(t.numel() - 1)
    if how == "more":
        return t.new_zeros(t.numel() + 1)
    if how == "meta":
        return torch.empty(t.shape, dtype=t.dtype, device="meta")
    return t.numpy()


def good(name):
    """The good operands of a wrapper, fresh tensors every time."""
    logits, mask, rec, prob = f32(1, 8, S, S), u8(F, H, W), i32(F, ops.DETECT_REC_WORDS), i16(F, H, W)
    video = u8(F, H, W, 3)
    if name == "truth_frame_flags":
        return dict(truth=u8(F, H, W), h0=0, w0=0, S=S, flags=i32(F))
    if name == "eval_clips_from_u8":
        return dict(video=video, truth=u8(F, H, W), h0=0, w0=0, S=S, starts=STARTS, out=(f32(1, 8, S, S, 4), f32(1, 8, S, S)))
    if name == "clips_from_u8":
        return dict(video=video, h0=0, w0=0, S=S, starts=STARTS, out=f32(1, 8, S, S, 4))
    if name == "clips_from_u8_views":
        return dict(video=video, views=VIEWS, S=S, starts=STARTS, out=f32(1, 1, 8, S, S, 4))
    if name == "video_vote":
        return dict(pred=f32(1, 3), label=0, n_correct=i32(1))
    if name == "video_class":
        return dict(scores=f32(1, 3), out=f32(5))
    if name == "detect_frames":
        return dict(logits=logits, starts=STARTS, F=F, H=H, W=W, h0=0, w0=0, mask=mask, rec=rec, ws=u8(ops.detect_frames_ws_bytes(1, S)))
    if name == "detect_frames_views":
        return dict(logits=logits, views=VIEWS, starts=STARTS, F=F, H=H, W=W, mask=mask, rec=rec, ws=u8(ops.detect_frames_views_ws_bytes(1, H, W)))
    if name == "detect_frames_scaled":
        return dict(logits=logits, views=VIEWS, starts=STARTS, F=F, H=H, W=W, Hs=H, Ws=W, mask=mask, prob=prob, rec=rec,
                    ws=u8(ops.detect_frames_scaled_ws_bytes(1, H, W, H, W)))
    if name == "clip_planes":
        return dict(logits=logits, views=VIEWS, starts=STARTS, F=F, Hs=H, Ws=W, f_skip=1, hop=4, planes=u8(ops.clip_planes_bytes(F, H, W, 1, 4)))
    if name == "detect_frames_planes":
        return dict(planes=u8(ops.clip_planes_bytes(F, H, W, 1, 4)), F=F, H=H, W=W, Hs=H, Ws=W, V=1, f_skip=1, hop=4, mask=mask, prob=prob, rec=rec,
                    ws=u8(ops.detect_frames_planes_ws_bytes(F, H, W)))
    if name == "frame_probs":
        return dict(logits=logits, views=VIEWS, starts=STARTS, F=F, H=H, W=W, prob=prob)
    if name == "frame_instances":
        return dict(mask=mask, K=K, inst=i32(F, ops.INST_HDR + K * ops.INST_WORDS), imap=u8(F, H, W))
    if name == "instance_scores":
        return dict(imap=u8(F, H, W), prob=prob, K=K, out=i32(F, ops.SCORE_WORDS * (K + 1)))
    if name == "instance_overlaps":
        return dict(imap=u8(F, H, W), K=K, L=L, out=i32(F, L, K + 1, K + 1))
    if name == "mask_run_index":
        return dict(map=u8(F, H, W), index=i32(F * H + 1))
    if name == "mask_runs":
        return dict(map=u8(F, H, W), index=i32(F * H + 1), cap=3, runs=i32(3, ops.RUN_WORDS))
    if name == "map_crosstab":
        return dict(pred=u8(F, H, W), truth=u8(F, H, W), P=P, A=A, out=i32(F, P + 2, A + 2), ws=u8(ops.map_crosstab_ws_bytes(F, H, W, P, A)))
    if name == "prob_truth_hist":
        return dict(prob=prob, truth=u8(F, H, W), words=WORDS, out=i32(F, 2, len(WORDS) + 1), ws=u8(ops.prob_truth_hist_ws_bytes(F, H, W, len(WORDS))))
    if name == "prob_cut":
        return dict(prob=prob, word=32768, mask=mask, rec=rec, ws=u8(ops.prob_cut_ws_bytes(F, H, W)))
    if name == "resize_u8":
        return dict(src=u8(1, H, W, 3), Ho=2, Wo=4, interpolation=1)
    raise KeyError(name)


# a flat tensor has no [-2] to read S from, so "one clip frame too few / too many" stands in for "fewer" / "more" on the logits
LOGITS = [(dict(logits=f32(7, S, S)), "V"), (dict(logits=f32(9, S, S)), "R")]

# wrapper -> (what the good operands end in, {operand: one letter per PERTURB}, [(scalar arguments, letter)]).  "out.0": element 0 of the tuple `out`.
TABLE = {
    "truth_frame_flags": ("R", {"truth": "VVVVRV", "flags": "VVVRRV"}, []),
    "eval_clips_from_u8": ("R", {"video": "VVVVVV", "truth": "VVVVRV", "out.0": "VVVRVV", "out.1": "VVVRVV"}, []),
    "clips_from_u8": ("R", {"video": "VVVVVV", "out": "VVVRVV"}, []),
    "clips_from_u8_views": ("R", {"video": "VVVVVV", "out": "VVVRVV"}, [(dict(view_stride=0), "V"), (dict(views=[]), "V")]),
    "video_vote": ("R", {"pred": "VVVVRV", "n_correct": "V-VRRV"}, []),
    "video_class": ("R", {"scores": "VVVVVV", "out": "VVVVVV"}, []),
    "detect_frames": ("R", {"logits": "VV--VV", "mask": "VVVVVV", "rec": "VVVVVV", "ws": "RVVRV-"}, LOGITS),
    "detect_frames_views": ("R", {"logits": "VV--VV", "mask": "VVVVVV", "rec": "VVVVVV", "ws": "RVVRV-"}, LOGITS + [(dict(view_stride=0), "V")]),
    "detect_frames_scaled": ("R", {"logits": "VV--VV", "mask": "VVVVVV", "prob": "VVVVVV", "rec": "VVVVVV", "ws": "RVVRV-"},
                             LOGITS + [(dict(H=0), "V")]),
    "clip_planes": ("R", {"logits": "VV--VV", "planes": "VVVRVV"}, LOGITS + [(dict(hop=3), "V"), (dict(F=0), "V")]),
    "detect_frames_planes": ("R", {"planes": "VVVRVV", "mask": "VVVVVV", "prob": "VVVVVV", "rec": "VVVVVV", "ws": "RVVRV-"},
                             [(dict(f0=-1), "V"), (dict(nf=0), "V"), (dict(f0=1, nf=F), "V"), (dict(nf=257), "V")]),
    "frame_probs": ("R", {"logits": "VV--VV", "prob": "VVVVVV"}, LOGITS),
    "frame_instances": ("R", {"mask": "VVVVVV", "inst": "VVVVVV", "imap": "VVVVVV"},
                        [(dict(K=0), "V"), (dict(K=33), "V"), (dict(f0=-1), "R"), (dict(nf=0), "R"), (dict(f0=1, nf=F), "R")]),
    "instance_scores": ("R", {"imap": "VVVVVV", "prob": "VVVVVV", "out": "VVVVVV"},
                        [(dict(K=0), "V"), (dict(K=33), "V"), (dict(prob=None), "V"), (dict(f0=-1), "R"), (dict(nf=0), "R")]),
    "instance_overlaps": ("R", {"imap": "VVVVVV", "out": "VVVVVV"},
                          [(dict(K=0), "V"), (dict(K=33), "V"), (dict(L=0), "V"), (dict(L=5), "V"), (dict(f0=-1), "R"), (dict(nf=0), "R")]),
    "mask_run_index": ("R", {"map": "VVVVVV", "index": "VVVVVV"}, [(dict(f0=-1), "V"), (dict(nf=0), "V"), (dict(f0=1, nf=F), "V")]),
    "mask_runs": ("R", {"map": "VVVVVV", "index": "VVVVVV", "runs": "VVVVVV"}, [(dict(f0=-1), "V"), (dict(nf=0), "V"), (dict(cap=-1, runs=None), "V")]),
    "map_crosstab": ("R", {"pred": "VVVVVV", "truth": "VVVVVV", "out": "VVVVVV", "ws": "VVVRVV"},
                     [(dict(P=0), "V"), (dict(A=33), "V"), (dict(f0=-1), "V"), (dict(nf=0), "V"), (dict(f0=1, nf=F), "V")]),
    "prob_truth_hist": ("R", {"prob": "VVVVVV", "truth": "VVVVVV", "out": "VVVVVV", "ws": "VVVRVV"},
                        [(dict(words=[]), "V"), (dict(words=[200, 100]), "V"), (dict(f0=-1), "V"), (dict(nf=0), "V"), (dict(f0=1, nf=F), "V")]),
    "prob_cut": ("V", {"prob": "VVVVVV", "mask": "VVVVVV", "rec": "VVVVVV", "ws": "VVVVVV"}, [(dict(word=0), "V"), (dict(f0=-1), "V"), (dict(nf=0), "V")]),
    "resize_u8": ("R", {"src": "VVVVRV"}, []),
}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def outcome(name, kwargs):
    """"V": the wrapper's ValueError, naming it; "R": ops.ptr's refusal of a CPU tensor; else the name of what was raised (or "returned")."""
    try:
        getattr(ops, name)(**kwargs)
    except ValueError as e:
        named = name in str(e) or (name == "detect_frames_planes" and "clip_planes" in str(e))       # its planes are checked under clip_planes' name
        return "V" if named else "ValueError without the wrapper's name: %s" % e
    except RuntimeError as e:
        return "R" if "no CPU fallback" in str(e) else "RuntimeError: %s" % e
    except Exception as e:               # noqa: BLE001  (the table says which cases may not end here)
        return type(e).__name__
    return "returned"


def with_operand(kwargs, operand, value):
    key, _, i = operand.partition(".")
    if i:
        items = list(kwargs[key])
        items[int(i)] = value
        value = tuple(items)
    return dict(kwargs, **{key: value})


def operand_of(kwargs, operand):
    key, _, i = operand.partition(".")
    return kwargs[key][int(i)] if i else kwargs[key]


def observed(name):
    """The row of `name` as the code at hand behaves: (good, {operand: letters}) -- "-" for a perturbation that does not exist or ends elsewhere."""
    row = {}
    for operand in TABLE[name][1]:
        letters = ""
        for how in PERTURB:
            bad = perturbed(operand_of(good(name), operand), how)
            got = "-" if bad is None else outcome(name, with_operand(good(name), operand, bad))
            letters += got if got in ("V", "R") else "-"
        row[operand] = letters
    return outcome(name, good(name)), row


def cases():
    for name, (_good, operands, scalars) in TABLE.items():
        yield name, None, None
        for operand, letters in operands.items():
            for how, letter in zip(PERTURB, letters):
                if letter != "-":
                    yield name, operand, how
        for i in range(len(scalars)):
            yield name, "scalars", i


CASES = list(cases())


@pytest.mark.parametrize("name,operand,how", CASES, ids=["-".join(str(x) for x in c if x is not None) for c in CASES])
def test_operand_case_ends_as_recorded(built, name, operand, how):
    want_good, operands, scalars = TABLE[name]
    if operand is None:
        assert outcome(name, good(name)) == want_good
    elif operand == "scalars":
        kw, want = scalars[how]
        assert outcome(name, dict(good(name), **kw)) == want, kw
    else:
        bad = perturbed(operand_of(good(name), operand), how)
        assert bad is not None
        assert outcome(name, with_operand(good(name), operand, bad)) == operands[operand][PERTURB.index(how)]


def test_every_wrapper_of_the_half_has_a_row():
    assert sorted(TABLE) == sorted(["truth_frame_flags", "eval_clips_from_u8", "clips_from_u8", "clips_from_u8_views", "video_vote", "video_class",
                                    "detect_frames", "detect_frames_views", "detect_frames_scaled", "clip_planes", "detect_frames_planes",
                                    "frame_probs", "frame_instances", "instance_scores", "instance_overlaps", "mask_run_index", "mask_runs",
                                    "map_crosstab", "prob_truth_hist", "prob_cut", "resize_u8"])
    assert all(len(letters) == len(PERTURB) for _g, operands, _s in TABLE.values() for letters in operands.values())


def test_fresh_buffers_are_made_where_none_is_given(built):
    """Every optional operand left out: the wrapper makes its own and still ends at ops.ptr (prob_cut: at its device check)."""
    for name, (want_good, _operands, _scalars) in TABLE.items():
        optional = [k for k, p in inspect.signature(getattr(ops, name)).parameters.items() if p.default is None]
        kw = {k: v for k, v in good(name).items() if k not in optional}
        assert outcome(name, kw) == want_good, name


# ---------------------------------------------------------------------- decode_*: numpy in, torch in, same arrays out
RNG = np.random.default_rng(7)


def _words(n):
    return RNG.integers(0, 1 << 20, n, dtype=np.int64).astype(np.int32)


DECODERS = [
    ("decode_val_record", lambda: np.concatenate([_words(9), np.int32([2]), _words(6)]), ()),
    ("decode_detect_records", lambda: _words(F * ops.DETECT_REC_WORDS).reshape(F, -1), ()),
    ("decode_instances", lambda: _words(F * (ops.INST_HDR + K * ops.INST_WORDS)).reshape(F, -1), (K,)),
    ("decode_instance_scores", lambda: _words(F * ops.SCORE_WORDS * (K + 1)), (K,)),
    ("decode_instance_overlaps", lambda: _words(F * L * (K + 1) ** 2), (K, L)),
    ("decode_map_crosstab", lambda: _words(F * (P + 2) * (A + 2)), (P, A)),
    ("decode_prob_truth_hist", lambda: _words(F * 2 * (len(WORDS) + 1)), (len(WORDS),)),
    ("decode_mask_runs", lambda: np.array([[1 | 1 << 24, 2 | 5 << 16], [6 | 3 << 24, 0 | 8 << 16]], np.int32), (F, H, W)),
]


def _flat(x):
    if isinstance(x, dict):
        return [v for _k, v in sorted(x.items())]
    return list(x) if isinstance(x, tuple) else [x]


@pytest.mark.parametrize("name,make,args", DECODERS, ids=[d[0] for d in DECODERS])
def test_decoders_take_numpy_and_torch_alike(name, make, args):
    words = make()
    keep = words.copy()
    a, b = _flat(getattr(ops, name)(words, *args)), _flat(getattr(ops, name)(torch.from_numpy(words.copy()), *args))
    assert len(a) == len(b) and np.array_equal(words, keep)
    for x, y in zip(a, b):
        assert type(x) is type(y) and np.array_equal(np.asarray(x), np.asarray(y))
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape


if __name__ == "__main__":
    capi.lib()
    for wrapper in TABLE:
        print(wrapper, *observed(wrapper))
        for kwargs, _want in TABLE[wrapper][2]:
            print("   ", kwargs, outcome(wrapper, dict(good(wrapper), **kwargs)))
