"""Training state checkpoints: everything a stopped run needs to go on bit for bit at an epoch boundary, in one file.

A training state is a plain dict (FORMAT / VERSION below): the reference-key model `state_dict`, the optimiser state in the
structure `torch.optim.Adam(...).state_dict()` has (per tensor, reference NCDHW layout, parameters in `named_parameters()` order --
so the fused engine, the nn.Module + autograd path and the reference's own `optim.Adam` can each continue what another wrote), the
`ReduceLROnPlateau` state, the last finished epoch, the best losses and checkpoint paths, the host RNG states and the run's arguments.

Everything here runs on the host and needs no GPU: the format, the conversions between the engine's flat moment buffers and the
per-tensor optimiser state, and the checks.  The position inside an epoch and DataLoader worker state are not part of a training state.
"""
import os
import random

import numpy as np
import torch

FORMAT = "picons_train_state"
VERSION = 1
TOP_KEYS = ("format", "version", "model", "optimizer", "scheduler", "epoch", "best", "rng", "args", "meta")
META_REFUSED = ("num_classes", "hw", "dataset", "world")          # check_compatible: a different value of one of these is refused

_template = None


def adam_template():
    """-> (step key, first-moment key, second-moment key, a step value, param_group fields) of the INSTALLED torch's Adam, read off a real
    one stepped once on a gradient of ones (first moment 1 - beta1, second 1 - beta2), not written down from memory."""
    global _template
    if _template is None:
        p = torch.nn.Parameter(torch.zeros(2, 3))
        opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0)
        p.grad = torch.ones(2, 3)
        opt.step()
        sd = opt.state_dict()
        st = sd["state"][0]
        moments = sorted((k for k, v in st.items() if torch.is_tensor(v) and tuple(v.shape) == (2, 3)), key=lambda k: -float(st[k].flatten()[0]))
        steps = [k for k, v in st.items() if k not in moments]
        if len(moments) != 2 or len(steps) != 1:
            raise RuntimeError("torch.optim.Adam's state has the keys %s: expected a step count and two moments" % sorted(st))
        group = {k: v for k, v in sd["param_groups"][0].items() if k != "params"}
        _template = (steps[0], moments[0], moments[1], st[steps[0]], group)
    return _template


def adam_param_group(lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0):
    """One Adam param_group (without `params`) with the installed torch's fields and defaults."""
    g = dict(adam_template()[4])
    g.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    return g


def _numel(shape):
    return int(np.prod(shape)) if len(shape) else 1


def _groups_for(param_groups, n):
    groups = [dict(g) for g in param_groups]
    if len(groups) == 1:
        groups[0]["params"] = list(range(n))
    elif sorted(i for g in groups for i in g.get("params", [])) != list(range(n)):
        raise ValueError("param_groups: %d groups must index the %d parameters between them" % (len(groups), n))
    return groups


def adam_state_from_flat(M, V, step_count, poff, pshape, names, param_groups):
    """Flat moment buffers -> the dict `torch.optim.Adam.state_dict()` writes: parameter i is names[i], its moments the slices
    [poff[name], poff[name] + numel) of M and V as host tensors of shape pshape[name].  step_count 0: no state yet, as a fresh Adam."""
    k_step, k_m, k_v, step0, _ = adam_template()
    state = {}
    if step_count:
        for i, name in enumerate(names):
            shp, o = tuple(pshape[name]), poff[name]
            n = _numel(shp)
            host = lambda buf: buf[o:o + n].detach().to("cpu", torch.float32, copy=True).view(shp)
            step = torch.full_like(step0, step_count) if torch.is_tensor(step0) else type(step0)(step_count)
            state[i] = {k_step: step, k_m: host(M), k_v: host(V)}
    return {"state": state, "param_groups": _groups_for(param_groups, len(names))}


def adam_state_check(opt_state, M, V, poff, pshape, names):
    """Everything adam_state_to_flat refuses, without writing: -> (step_count, [(name, first moment, second moment)])."""
    k_step, k_m, k_v, _, _ = adam_template()
    try:
        state = opt_state["state"]
        state.keys()
    except (KeyError, TypeError, AttributeError):
        raise ValueError("optimizer state: a dict with a 'state' dict expected, got %s" % type(opt_state).__name__) from None
    n_names = len(names)
    if len(state) == 0:                 # an optimiser that has not stepped
        todo, count = [(name, None, None) for name in names], 0
    else:
        if len(state) != n_names or sorted(state, key=str) != sorted(range(n_names), key=str):
            missing = [names[i] for i in range(n_names) if i not in state][:3]
            raise ValueError("optimizer state holds %d tensors, this engine has %d parameters%s"
                             % (len(state), n_names, (" (missing: %s ...)" % ", ".join(missing)) if missing else ""))
        todo, count = [], None
        for i, name in enumerate(names):
            st = state[i]
            for k in (k_step, k_m, k_v):
                if k not in st:
                    raise ValueError("optimizer state of %s has no %r" % (name, k))
            shp = tuple(pshape[name])
            for k in (k_m, k_v):
                if not torch.is_tensor(st[k]) or tuple(st[k].shape) != shp:
                    got = tuple(st[k].shape) if torch.is_tensor(st[k]) else type(st[k]).__name__
                    raise ValueError("optimizer state of %s: %s has shape %s, the parameter %s" % (name, k, got, shp))
                if not bool(torch.isfinite(st[k]).all()):
                    raise ValueError("optimizer state of %s: %s holds a non-finite value" % (name, k))
            step = float(st[k_step])
            if not np.isfinite(step) or step < 0 or step != int(step):
                raise ValueError("optimizer state of %s: step is %r, a whole number of steps expected" % (name, step))
            if count is None:
                count = int(step)
            elif int(step) != count:
                raise ValueError("optimizer state of %s: step %d, but %s is at step %d (the fused step keeps one count for all)"
                                 % (name, int(step), names[0], count))
            todo.append((name, st[k_m], st[k_v]))
    for name in names:
        o, n = poff[name], _numel(tuple(pshape[name]))
        if o < 0 or o + n > M.numel() or o + n > V.numel():
            raise ValueError("%s at [%d, %d) does not fit the flat buffers of %d / %d floats" % (name, o, o + n, M.numel(), V.numel()))
    return count, todo


def adam_state_to_flat(opt_state, M, V, poff, pshape, names):
    """The inverse of adam_state_from_flat: per-tensor optimiser state into the flat buffers; -> step_count.  Everything is validated first --
    tensor count, shapes, one step count for all, finite values -- and a refusal (ValueError naming the tensor) has written nothing.
    Elements of M / V outside every named tensor are left as they are."""
    count, todo = adam_state_check(opt_state, M, V, poff, pshape, names)
    with torch.no_grad():
        for name, m, v in todo:
            o, n = poff[name], _numel(tuple(pshape[name]))
            if m is None:
                M[o:o + n].zero_()
                V[o:o + n].zero_()
            else:
                M[o:o + n].copy_(m.detach().reshape(-1))
                V[o:o + n].copy_(v.detach().reshape(-1))
    return count


def _is_array(v):
    return torch.is_tensor(v) or isinstance(v, np.ndarray)


def model_state_of(obj):
    """What a checkpoint file holds -> the model `state_dict` in it.  A bare state_dict (names -> tensors) is returned as is, a training state
    gives its `model`; anything else is a ValueError that says what was found -- `load_state_dict(..., strict=False)` would load nothing from
    it without a word."""
    if not isinstance(obj, dict):
        raise ValueError("not a checkpoint: a state_dict or a %s dict expected, got %s" % (FORMAT, type(obj).__name__))
    if "format" in obj:
        if obj["format"] != FORMAT:
            raise ValueError("checkpoint has format %r, expected %r" % (obj["format"], FORMAT))
        if obj.get("version") != VERSION:
            raise ValueError("%s checkpoint has version %r, this code reads version %d" % (FORMAT, obj.get("version"), VERSION))
        if not isinstance(obj.get("model"), dict):
            raise ValueError("%s checkpoint without a 'model' state_dict" % FORMAT)
        return obj["model"]
    if len(obj) and all(isinstance(k, str) for k in obj) and all(_is_array(v) for v in obj.values()):
        return obj
    odd = [k for k, v in obj.items() if not (isinstance(k, str) and _is_array(v))]
    raise ValueError("neither a state_dict nor a %s checkpoint: a dict of %d entries%s"
                     % (FORMAT, len(obj), (", of which %s are not tensors" % [str(k) for k in odd[:5]]) if odd else ""))


def check_format(state):
    """Format, version and top-level keys of a training state; -> state."""
    if not isinstance(state, dict) or "format" not in state:
        raise ValueError("not a %s checkpoint: %s" % (FORMAT, ("a dict with the keys %s" % sorted(map(str, state))[:6]) if isinstance(state, dict)
                                                      else type(state).__name__))
    model_state_of(state)
    missing = [k for k in TOP_KEYS if k not in state]
    if missing:
        raise ValueError("%s checkpoint lacks %s" % (FORMAT, missing))
    return state


def save(path, state):
    """Write `state` to `path` through a temporary file in the same directory and one os.replace: a failure while writing leaves an existing
    `path` as it was and no temporary file behind."""
    tmp = path + ".tmp"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def load(path):
    """-> the training state in `path` (host tensors), its format, version and top-level keys checked."""
    return check_format(torch.load(path, map_location="cpu"))


def check_compatible(state, meta, args=None):
    """Refuse (ValueError) a training state written for another num_classes / hw / dataset / world (the per-rank RNG states exist only for
    the world that wrote them); a different `fused` is allowed -- the optimiser state is per tensor so that either path continues the other.
    -> [(flag, saved, now)] for the arguments (args: this run's, a dict or a namespace) that differ from the saved ones, for the caller to
    print (arg_warning): not refused, extending --epochs is legitimate."""
    saved = state["meta"]
    for k in META_REFUSED:
        if saved.get(k) != meta.get(k):
            raise ValueError("training state was written with %s=%r, this run has %s=%r" % (k, saved.get(k), k, meta.get(k)))
    if args is None:
        return []
    now = dict(args) if isinstance(args, dict) else dict(vars(args))
    old = state["args"]
    return [(k, old.get(k), now.get(k)) for k in sorted(set(old) | set(now)) if old.get(k) != now.get(k)]


def arg_warning(diffs):
    """The text a trainer prints for check_compatible's differences."""
    lines = ["WARNING: resuming with --%s %r (the state was written with %r)" % (k, now, old) for k, old, now in diffs]
    if any(k == "epochs" for k, _, _ in diffs):
        lines.append("WARNING: a different --epochs changes exp_rampup's ramp: the consistency weight of every remaining epoch differs from the "
                     "one the interrupted run would have used")
    return "\n".join(lines)


def rng_state(torch_states=None, cuda_states=None):
    """The host RNGs a trainer draws from, in types torch.load reads back with weights_only: python's and numpy's global generators and torch's
    CPU generator (torch_states: one per rank, gathered by the caller; default this process's alone)."""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    st = {"python": random.getstate(),
          "numpy": (str(kind), torch.from_numpy(np.asarray(keys).astype(np.int64)), int(pos), int(has_gauss), float(cached)),
          "torch": [torch.get_rng_state()] if torch_states is None else list(torch_states)}
    if cuda_states is not None:
        st["cuda"] = list(cuda_states)
    return st


def _tuples(x):
    return tuple(_tuples(v) for v in x) if isinstance(x, (list, tuple)) else x


def set_rng_state(rng, rank=0):
    random.setstate(_tuples(rng["python"]))
    kind, keys, pos, has_gauss, cached = rng["numpy"]
    np.random.set_state((kind, np.asarray(keys).astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    if rank >= len(rng["torch"]):
        raise ValueError("training state holds the RNG states of %d ranks, this is rank %d" % (len(rng["torch"]), rank))
    torch.set_rng_state(rng["torch"][rank])
    cuda = rng.get("cuda")
    if cuda is not None and rank < len(cuda) and cuda[rank] is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(cuda[rank])
