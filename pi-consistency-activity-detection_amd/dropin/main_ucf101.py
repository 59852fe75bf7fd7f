#!/usr/bin/env python3
"""Drop-in for /root/reference/main_ucf101.py: same CLI flags (:285-315), same train/validate loop
structure and checkpoint policy (:434-456), same `train_model_interface` contract (:50-150) - with the
model, the bv/gv masks and the optimiser step running on MI355X HIP kernels.

New behaviour is switched by environment variables only, so the CLI is unchanged:
  PICONS_SYNTHETIC=1     synthetic UCF101-24-shaped minibatches (no dataset / decoder libs on the box)
  PICONS_SYNTHETIC=u8    synthetic decoded uint8 videos + box annotations through the device input pipeline (picons_amd.inputpipe)
  PICONS_SYNTHETIC=0     the caller's datasets from PYTHONPATH (datasets.ucf_dataloader.UCF101DataLoader; for JHMDB
                         datasets.load_jhmdb_pytorch_multi.JHMDB) in the reference's DataLoaders (real_loaders)
  PICONS_STEPS=<n>       steps per epoch in synthetic mode (default 4)
  PICONS_LABELED_CLIPS=<n>    synthetic mode: the labeled set has n clips, batched like DataLoader(batch_size=bs // 2, drop_last=False)
  PICONS_UNLABELED_CLIPS=<n>  the same for the unlabeled set; it sets the steps per epoch (PICONS_STEPS is then not used).  Unset: every
                         batch is full (bs // 2 clips) and an epoch is PICONS_STEPS steps
  PICONS_FUSED=0         use the nn.Module + autograd path (model called twice, torch.optim.Adam) instead of
                         the fused step engine (default 1: picons_amd.step.StepEngine, both passes batched)
  PICONS_HW=<px>         frame size (default 224, the only size the reference accepts)
  PICONS_TRAIN_STATE=<path>   after every epoch (behind the scheduler step) rank 0 writes the whole training state to <path>
                         (picons_amd.trainstate: model, Adam moments per tensor as torch.optim.Adam.state_dict() has them, scheduler, epoch, best
                         losses and checkpoint paths, the host RNG states of every rank, the arguments), atomically.  Unset: no such file
  PICONS_RESUME=<path>   continue the run that wrote <path> at its next epoch, in its checkpoint directory, bit for bit as if it had
                         not stopped (same --bs / data / world; either PICONS_FUSED path continues the other's file).  Epoch boundaries
                         only: the position inside an epoch and DataLoader worker state are not saved
  PICONS_EPOCHS_THIS_RUN=<n>  stop cleanly after n epochs of this invocation (for time-limited job slots; --epochs stays the run's length)
  RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*   data parallel over the GPUs of one node (torchrun)
"""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bootstrap  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from torch import optim  # noqa: E402

from models.capsules_ucf101 import CapsNet  # noqa: E402
from utils.losses import SpreadLoss, DiceLoss, weighted_mse_loss  # noqa: E402
from utils.metrics import get_accuracy, IOU2  # noqa: E402
from utils.helpers import measure_pixelwise_var_v2, measure_pixelwise_gradient  # noqa: E402
from utils import ramp_ups  # noqa: E402
from picons_amd import dist as pdist, step as pstep, synthetic, trainstate, valstep as pval  # noqa: E402

NUM_CLASSES = 24
DATASET = "ucf101"
model = criterion_cls = criterion_seg_1 = criterion_seg_2 = None


def _dev(t, dtype=None):
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    return t.cuda().to(dtype) if dtype is not None else t.cuda()


def val_model_interface(minibatch):
    """main_ucf101.py:33-47."""
    data = _dev(minibatch['data'], torch.float32)
    action = _dev(minibatch['action'])
    segmentation = _dev(minibatch['loc_msk'], torch.float32)
    empty_vector = torch.zeros(action.shape[0]).cuda()
    output, predicted_action, _ = model(data, action, empty_vector, 0, 0)
    class_loss, abs_class_loss = criterion_cls(predicted_action, action)
    loss1 = criterion_seg_1(output, segmentation)
    loss2 = criterion_seg_2(output, segmentation)
    loc_loss = loss1 + loss2
    total_loss = loc_loss + class_loss
    return (output, predicted_action, segmentation, action, total_loss, loc_loss, class_loss)


def train_model_interface(args, label_minibatch, unlabel_minibatch, epoch, wt_ramp):
    """main_ucf101.py:50-150 on the nn.Module path (two forward calls, autograd)."""
    cat = lambda k, dt=None: torch.cat([_dev(label_minibatch[k], dt), _dev(unlabel_minibatch[k], dt)], dim=0)
    concat_data = cat('data', torch.float32)
    concat_fl_data = cat('aug_data', torch.float32)
    concat_action = cat('action')
    concat_seg = cat('loc_msk', torch.float32)
    if DATASET == "jhmdb":            # main_jhmdb.py:68-70
        concat_labels = torch.cat([torch.ones(len(label_minibatch['action'])), torch.zeros(len(unlabel_minibatch['action']))]).cuda()
    else:
        concat_labels = cat('label_vid')
    random_indices = torch.randperm(len(concat_labels)).cuda()
    concat_data, concat_fl_data = concat_data[random_indices], concat_fl_data[random_indices]
    concat_action, concat_labels, concat_seg = concat_action[random_indices], concat_labels[random_indices], concat_seg[random_indices]
    labeled_vid_index = torch.where(concat_labels == 1)[0]

    output, predicted_action, feat = model(concat_data, concat_action, concat_labels, epoch, args.thresh_epoch)
    flip_op, _, _ = model(concat_fl_data, concat_action, concat_labels, epoch, args.thresh_epoch)

    labeled_op = output[labeled_vid_index]
    labeled_seg_data = concat_seg[labeled_vid_index]
    loc_loss = criterion_seg_1(labeled_op, labeled_seg_data) + criterion_seg_2(labeled_op, labeled_seg_data)
    class_loss, abs_class_loss = criterion_cls(predicted_action[labeled_vid_index], concat_action[labeled_vid_index])

    flipped_pred_seg_map = torch.flip(flip_op, [4])
    loss_wt_simple_l2 = weighted_mse_loss(flipped_pred_seg_map, output, torch.ones_like(output))
    total_seg_cons_loss_1 = total_seg_cons_loss_2 = None
    if args.bv:
        v_c = measure_pixelwise_var_v2(output, torch.flip(flipped_pred_seg_map, [2]), frames_cnt=args.n_frames, use_sig_output=args.predict_maps)
        v_a = measure_pixelwise_var_v2(torch.flip(output, [2]), flipped_pred_seg_map, frames_cnt=args.n_frames, use_sig_output=args.predict_maps)
        loss_wt_var_1 = weighted_mse_loss(flipped_pred_seg_map, output, v_c)
        loss_wt_var_2 = weighted_mse_loss(flipped_pred_seg_map, output, torch.flip(v_a, [2]))
        total_seg_cons_loss_1 = (wt_ramp * (loss_wt_var_1 + loss_wt_var_2)) + ((1 - wt_ramp) * loss_wt_simple_l2)
    if args.gv:
        batch_grad = measure_pixelwise_gradient(output, conf_thresh_lower=args.lower_thresh, conf_thresh_upper=args.upper_thresh)
        total_seg_cons_loss_2 = weighted_mse_loss(flipped_pred_seg_map, output, batch_grad)
    if DATASET == "jhmdb":
        total_cons_loss = total_seg_cons_loss_2 if args.gv else (total_seg_cons_loss_1 if args.bv else loss_wt_simple_l2)
    elif args.bv and args.gv:
        total_cons_loss = args.bv_wt * total_seg_cons_loss_1 + args.gv_wt * total_seg_cons_loss_2
    elif args.gv:
        total_cons_loss = total_seg_cons_loss_2
    elif args.bv:
        total_cons_loss = total_seg_cons_loss_1
    else:
        total_cons_loss = loss_wt_simple_l2
    total_loss = args.wt_loc * loc_loss + args.wt_cls * class_loss + args.wt_cons * total_cons_loss
    return (output, predicted_action, concat_seg, concat_action, total_loss, loc_loss, class_loss, total_cons_loss)


class SyntheticLoader:
    """Stands in for torch DataLoader(UCF101DataLoader(...)) with the same minibatch dict contract.  items=None: `steps` batches of n
    clips; items=k: the batches of DataLoader(batch_size=n, drop_last=False) over k clips (the last one short when n does not divide k)."""

    def __init__(self, n, labeled, steps, rank, num_classes, hw, salt, items=None):
        self.n, self.labeled, self.steps, self.rank, self.nc, self.hw, self.salt = n, labeled, steps, rank, num_classes, hw, salt
        self.items = items

    def batch_sizes(self):
        if self.items is None:
            return [self.n] * self.steps
        return [min(self.n, self.items - i) for i in range(0, self.items, self.n)]

    def __len__(self):
        return len(self.batch_sizes())

    def __iter__(self):
        for i, m in enumerate(self.batch_sizes()):
            mb = synthetic.make_minibatch(m, self.labeled, (1234 + self.rank) * 7919 + 2 * i + self.salt, self.nc, self.hw)
            yield {k: torch.from_numpy(v) for k, v in mb.items()}


class SyntheticVideoLoader(SyntheticLoader):
    """PICONS_SYNTHETIC=u8: synthetic DECODED videos (uint8 frames + box annotations, what `load_video` has after `vread`) go
    through the device input pipeline (picons_amd.inputpipe.get_item = UCF101DataLoader.__getitem__ from that point on) and are
    collated like torch's default collate does, as device fp32 tensors."""

    def __iter__(self):
        from picons_amd import inputpipe
        for i, m in enumerate(self.batch_sizes()):
            samples = []
            for j in range(m):
                frames, ann = synthetic.make_decoded_video(((1234 + self.rank) * 7919 + 2 * i + self.salt) * 64 + j, self.labeled, self.nc)
                samples.append(inputpipe.get_item(frames, ann, train=True))
            yield {'data': torch.stack([s['data'] for s in samples]), 'aug_data': torch.stack([s['aug_data'] for s in samples]),
                   'loc_msk': torch.stack([s['loc_msk'] for s in samples]), 'action': torch.stack([s['action'] for s in samples]),
                   'label_vid': torch.tensor([s['label_vid'] for s in samples])}


def real_loaders(args, rank=0, world=1):
    """PICONS_SYNTHETIC=0: the caller's datasets, imported from PYTHONPATH as the reference imports them, in the DataLoaders of
    main_ucf101.py:345-372 (bs // 2 clips per train batch, shuffled, no drop_last -- so each train loader may end on a short batch --
    and bs per validation batch).  JHMDB (main_jhmdb.py:338-363) imports datasets.load_jhmdb_pytorch_multi.JHMDB, a module the reference
    tree does not ship: the caller supplies it, and its absence is an ImportError naming it.  Data parallel (WORLD_SIZE > 1): every rank
    loads its own contiguous shard of each set (pdist.shard_indices through a Subset, DistributedSampler-style without padding) and
    shuffles within it."""
    from torch.utils.data import DataLoader, Subset
    if DATASET == "jhmdb":
        try:
            from datasets.load_jhmdb_pytorch_multi import JHMDB
        except ImportError as e:
            raise ImportError("PICONS_SYNTHETIC=0 for JHMDB imports datasets.load_jhmdb_pytorch_multi (class JHMDB, main_jhmdb.py:338) from "
                              "PYTHONPATH; it is not importable: %s" % e) from e
        labeled = JHMDB('train', [224, 224], file_id=args.pkl_file_label, use_random_start_frame=False)
        unlabeled = JHMDB('train', [224, 224], file_id=args.pkl_file_unlabel, use_random_start_frame=False)
        val = JHMDB('test', [224, 224], file_id='testlist.txt', use_random_start_frame=False)
    else:
        from datasets.ucf_dataloader import UCF101DataLoader          # the caller's loader (needs skvideo / the dataset)
        labeled = UCF101DataLoader('train', [224, 224], file_id=args.pkl_file_label, use_random_start_frame=False)
        unlabeled = UCF101DataLoader('train', [224, 224], file_id=args.pkl_file_unlabel, use_random_start_frame=False)
        val = UCF101DataLoader('validation', [224, 224], file_id="test_annots.pkl", use_random_start_frame=False)
    print(len(labeled), len(unlabeled), len(val))
    if world > 1:
        labeled, unlabeled, val = (Subset(d, pdist.shard_indices(len(d), rank, world)) for d in (labeled, unlabeled, val))
    return (DataLoader(dataset=labeled, batch_size=args.bs // 2, num_workers=args.workers, shuffle=True),
            DataLoader(dataset=unlabeled, batch_size=args.bs // 2, num_workers=args.workers, shuffle=True),
            DataLoader(dataset=val, batch_size=args.bs, num_workers=args.workers, shuffle=False))


def synthetic_loaders(args, mode, hw, rank=0, world=1):
    """PICONS_SYNTHETIC=1 / u8: stand-ins for the three loaders.  PICONS_LABELED_CLIPS / PICONS_UNLABELED_CLIPS give the train sets a
    size (this rank's shard of it), batched as the reference's DataLoaders batch it."""
    n = args.bs // 2
    steps = int(os.environ.get("PICONS_STEPS", "4"))
    clips = lambda key: None if os.environ.get(key) is None else len(pdist.shard_indices(int(os.environ[key]), rank, world))
    Loader = SyntheticVideoLoader if (mode == "u8" and hw == 224 and DATASET == "ucf101") else SyntheticLoader
    labeled_loader = Loader(n, True, steps, rank, NUM_CLASSES, hw, 0, items=clips("PICONS_LABELED_CLIPS"))
    unlabeled_loader = Loader(n, False, steps, rank, NUM_CLASSES, hw, 1, items=clips("PICONS_UNLABELED_CLIPS"))
    val_loader = SyntheticLoader(args.bs, True, 1, rank, NUM_CLASSES, hw, 5)
    return labeled_loader, unlabeled_loader, val_loader


def train(args, model, labeled_train_loader, unlabeled_train_loader, optimizer, epoch, save_path, writer, ramp_wt, engine=None, reducer=None):
    """main_ucf101.py:155-223."""
    model.train(mode=True)
    model.training = True
    total_loss, accuracy, loc_loss, class_loss, class_consistency_loss = [], [], [], [], []
    steps = len(unlabeled_train_loader)
    start_time = time.time()
    labeled_iterloader = iter(labeled_train_loader)
    for batch_id, unlabel_minibatch in enumerate(unlabeled_train_loader):
        try:
            label_minibatch = next(labeled_iterloader)
        except StopIteration:
            labeled_iterloader = iter(labeled_train_loader)
            label_minibatch = next(labeled_iterloader)
        if engine is not None:            # fused HIP step: both passes batched, losses + Adam on device
            bs = len(label_minibatch['action']) + len(unlabel_minibatch['action'])
            perm = torch.randperm(bs).numpy()
            drops = [(torch.rand(bs, c) < 0.5).float().numpy() * 2 for c in (832, 128, 832, 128)]
            s = engine.train_step(label_minibatch, unlabel_minibatch, epoch, ramp_wt(epoch), perm, drops, lr=optimizer.param_groups[0]['lr'], reducer=reducer)
            _out, _flip, pred = engine.outputs()
            total_loss.append(s['total']); loc_loss.append(s['loc']); class_loss.append(s['cls']); class_consistency_loss.append(s['cons'])
            accuracy.append(get_accuracy(pred, engine.action_host))
        else:
            optimizer.zero_grad()
            output, predicted_action, segmentation, action, loss, s_loss, c_loss, cc_loss = \
                train_model_interface(args, label_minibatch, unlabel_minibatch, epoch, ramp_wt(epoch))
            loss.backward()
            optimizer.step()
            total_loss.append(loss.item()); loc_loss.append(s_loss.item()); class_loss.append(c_loss.item())
            class_consistency_loss.append(cc_loss.item()); accuracy.append(get_accuracy(predicted_action, action))
        if (batch_id + 1) % args.pf == 0:
            print(f'[TRAIN] epoch-{epoch:0{len(str(args.epochs))}}/{args.epochs}, batch-{batch_id+1:0{len(str(steps))}}/{steps},'
                  f'loss-{np.mean(total_loss):.3f}, acc-{np.mean(accuracy):.3f}'
                  f'\t [LOSS ] cls-{np.mean(class_loss):.3f}, seg-{np.mean(loc_loss):.3f}, const-{np.mean(class_consistency_loss):.3f}')
            sys.stdout.flush()
    print("Training time: ", time.time() - start_time)
    return float(np.array(total_loss).mean())


def validate(model, val_data_loader, epoch, engine=None):
    """main_ucf101.py:226-278.  engine (picons_amd.valstep.ValEngine): the pass runs on the device -- forward, losses, IoU sums and accuracy
    per batch with no host round trip, one read-back at the end."""
    if engine is not None:
        engine.begin()
        for minibatch in val_data_loader:
            engine.val_step(minibatch)
        s = pval.summarize(engine.results(), epoch)
        print(s['line'])
        return s['total']
    model.eval()
    model.training = False
    total_loss, accuracy, total_IOU, validiou = [], [], 0, 0
    with torch.no_grad():
        for minibatch in val_data_loader:
            output, predicted_action, segmentation, action, loss, s_loss, c_loss = val_model_interface(minibatch)
            total_loss.append(loss.item())
            accuracy.append(get_accuracy(predicted_action, action))
            maskout_np = (output.cpu().numpy() > 0).astype(np.float32)
            truth_np = segmentation.cpu().numpy()
            for a in range(maskout_np.shape[0]):
                iou = IOU2(truth_np[a], maskout_np[a])
                if iou == iou:
                    total_IOU += iou; validiou += 1
    print(f'[VAL] epoch-{epoch}, loss-{np.mean(total_loss):.3f}, acc-{np.mean(accuracy):.3f} [IOU ] {total_IOU / max(validiou, 1):.3f}')
    return float(np.mean(total_loss))


# (flag, type or None for a switch, default, what it does) -- names, types and defaults are the reference's CLI
# (main_ucf101.py:285-315, main_jhmdb.py:283-310); the descriptions are this project's.
_COMMON_FLAGS = [
    ("bs", int, 16, "clips per step; half of them labeled, half unlabeled"),
    ("epochs", int, 1, "passes over the unlabeled set; also the length of the consistency ramp-up"),
    ("model_name", str, "i3d", "accepted for compatibility, not used"),
    ("lr", float, 0.001, "Adam step size at the start (ReduceLROnPlateau lowers it)"),
    ("pf", int, 50, "print running means every this many steps"),
    ("exp_id", str, "debug", "sub-directory of train_log_wts/ for checkpoints"),
    ("const_loss", str, "l2", "must be one of jsd / l2 / l1; the step always uses the L2 form, as the reference does"),
    ("wt_cls", float, 1, "weight of the spread (classification) loss"),
    ("wt_cons", float, 1, "weight of the flip-consistency loss"),
    ("seed", int, 47, "seeds python / numpy / torch RNGs"),
    ("thresh_epoch", int, 11, "from this epoch on unlabeled clips are masked with their predicted class instead of all classes"),
    ("n_frames", int, 3, "temporal window (3 or 5 frames) of the variance attention mask"),
    ("bv", None, False, "weight the consistency loss with the temporal-variance attention mask"),
    ("predict_maps", None, False, "take the variance of sigmoid(logits) instead of the logits"),
    ("cyclic", None, False, "accepted for compatibility, not used"),
    ("gv", None, False, "weight the consistency loss with the second-order temporal-gradient mask"),
    ("lower_thresh", float, None, "gradient mask: probabilities below this count as 0"),
    ("upper_thresh", float, None, "gradient mask: probabilities above this count as 1"),
]


def build_parser(extra):
    parser = argparse.ArgumentParser(description="semi-supervised action detection: flip consistency with variance / gradient attention")
    for name, typ, default, text in _COMMON_FLAGS + extra:
        if typ is None:
            parser.add_argument("--" + name, action="store_true", help=text)
        else:
            parser.add_argument("--" + name, type=typ, default=default, help=text)
    return parser


def parse_args(argv=None):
    """The flag set of main_ucf101.py:285-315."""
    return build_parser([
        ("pretrained", str, "i3d", "accepted for compatibility, not used"),
        ("loc_loss", str, "dice", "localisation loss next to BCE; only 'dice' exists"),
        ("pkl_file_label", str, "train_annots_20_labeled.pkl", "annotation file of the labeled split"),
        ("pkl_file_unlabel", str, "train_annots_80_unlabeled.pkl", "annotation file of the unlabeled split"),
        ("wt_loc", float, 1, "weight of the localisation (BCE + Dice) loss"),
        ("workers", int, 8, "DataLoader worker processes"),
        ("bv_wt", float, 0.5, "share of the variance-mask term when --bv and --gv are both given"),
        ("gv_wt", float, 0.5, "share of the gradient-mask term when --bv and --gv are both given"),
    ]).parse_args(argv)


def _host(x):
    """A state_dict-like structure with every tensor on the host."""
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_host(v) for v in x)
    return x


def _abs(path):
    """Paths go into a training state absolute: the run that resumes it may start in another working directory."""
    return None if path is None else os.path.abspath(path)


def _run_meta(world, hw, fused):
    return dict(num_classes=NUM_CLASSES, hw=hw, dataset=DATASET, world=world, fused=fused)


def write_train_state(path, args, meta, rank, epoch, model, optimizer, scheduler, engine, best):
    """PICONS_TRAIN_STATE: called by every rank behind an epoch's scheduler step (the RNG states of all ranks are gathered); rank 0 writes."""
    mine = (torch.get_rng_state(), torch.cuda.get_rng_state())
    gathered = [mine]
    if meta["world"] > 1:
        gathered = [None] * meta["world"]
        torch.distributed.all_gather_object(gathered, mine)
    if rank != 0:
        return
    if engine is not None:
        ts = engine.train_state()
        model_state, opt_state = ts["model"], ts["optimizer"]
        opt_state["param_groups"] = _host(optimizer.state_dict()["param_groups"])       # the learning rate lives in the torch optimiser
    else:
        model_state, opt_state = _host(model.state_dict()), _host(optimizer.state_dict())
    trainstate.save(path, {"format": trainstate.FORMAT, "version": trainstate.VERSION, "model": model_state, "optimizer": opt_state,
                           "scheduler": _host(scheduler.state_dict()), "epoch": epoch, "best": dict(best),
                           "rng": trainstate.rng_state([g[0] for g in gathered], [g[1] for g in gathered]),
                           "args": dict(vars(args)), "meta": dict(meta)})


def restore_train_state(state, model, optimizer, scheduler, engine, reducer):
    """PICONS_RESUME, on every rank: model, optimiser (fused: the engine's moments and step count, and the torch optimiser's param_groups
    alone), scheduler.  The RNG states are put back by the caller, last, behind everything that draws while the run is set up."""
    model.load_state_dict(state["model"])
    if engine is not None:
        engine.load_train_state(state)
        sd = optimizer.state_dict()
        sd["param_groups"] = [dict(g, params=mine["params"]) for g, mine in zip(state["optimizer"]["param_groups"], sd["param_groups"])]
        optimizer.load_state_dict(sd)
        if reducer is not None:
            pdist.check_replicas_agree(engine.P)
    else:
        optimizer.load_state_dict(state["optimizer"])
    scheduler.load_state_dict(state["scheduler"])


def run(args):
    global model, criterion_cls, criterion_seg_1, criterion_seg_2
    if args.loc_loss != 'dice':
        print("--loc_loss %r is not available (only 'dice'); stopping" % args.loc_loss)      # 'iou' is a NameError in the reference (:396)
        sys.exit(1)
    if args.const_loss not in ('jsd', 'l2', 'l1'):
        print("--const_loss %r is not one of jsd / l2 / l1; stopping" % args.const_loss)
        sys.exit(1)
    rank, world, local = pdist.init_from_env()
    torch.cuda.set_device(local)
    if args.seed:
        random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed + rank)
    hw = int(os.environ.get("PICONS_HW", "224"))
    fused = os.environ.get("PICONS_FUSED", "1") != "0"
    mode = os.environ.get("PICONS_SYNTHETIC", "1")          # read only: the process environment is not written to
    if mode not in ("0", "1", "u8"):
        raise RuntimeError("PICONS_SYNTHETIC=%r: expected 0 (the caller's datasets), 1 or u8" % mode)
    state_path, resume_path = os.environ.get("PICONS_TRAIN_STATE"), os.environ.get("PICONS_RESUME")
    epochs_this_run = int(os.environ.get("PICONS_EPOCHS_THIS_RUN", "0"))
    meta = _run_meta(world, hw, fused)
    resumed = None
    if resume_path:
        resumed = trainstate.load(resume_path)
        diffs = trainstate.check_compatible(resumed, meta, args)
        if diffs and rank == 0:
            print(trainstate.arg_warning(diffs), file=sys.stderr)
        if resumed["epoch"] >= args.epochs:
            print("PICONS_RESUME=%s: epoch %d of --epochs %d is finished, nothing left to train" % (resume_path, resumed["epoch"], args.epochs))
            return None
    if args.bs < 2:
        raise RuntimeError("--bs %d: each train loader takes bs // 2 clips per batch, so bs must be at least 2" % args.bs)
    if mode == "0":
        if hw != 224:
            raise RuntimeError("PICONS_SYNTHETIC=0: the reference's loaders make 224x224 clips; PICONS_HW=%d is for synthetic data" % hw)
        labeled_loader, unlabeled_loader, val_loader = real_loaders(args, rank, world)
    else:
        labeled_loader, unlabeled_loader, val_loader = synthetic_loaders(args, mode, hw, rank, world)
    print(len(labeled_loader), len(unlabeled_loader), len(val_loader))

    # the reference's CapsNet() loads ../weights/rgb_charades.pt and raises without it (capsules_ucf101.py:344).  In synthetic mode a
    # missing file is expected (no network for the download): pt_path=None is passed EXPLICITLY, so a caller who supplies the weights, or
    # constructs CapsNet() himself, still gets the hard error for a wrong path
    pt_path = '../weights/rgb_charades.pt'
    if not os.path.exists(pt_path):
        print("WARNING: %s not found (PICONS_SYNTHETIC=%s): the I3D trunk keeps its random initialisation" % (pt_path, mode), file=sys.stderr)
        pt_path = None
    model = CapsNet(pt_path=pt_path, num_classes=NUM_CLASSES, hw=hw, seed=args.seed) if NUM_CLASSES != 24 or hw != 224 else CapsNet(pt_path=pt_path, seed=args.seed)
    model = model.cuda()
    criterion_cls = SpreadLoss(num_class=NUM_CLASSES, m_min=0.2, m_max=0.9)
    criterion_seg_1 = nn.BCEWithLogitsLoss()
    criterion_seg_2 = DiceLoss()
    optimizer = optim.Adam(model.parameters(), lr=args.lr, weight_decay=0, eps=1e-6)
    scheduler = optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'min', min_lr=1e-7, patience=5, factor=0.1)
    ramp_wt = ramp_ups.exp_rampup(args.epochs)
    engine = reducer = val_engine = None
    if world > 1 and not fused:
        # the nn.Module path has no gradient exchange: N ranks would train N independent models and rank 0's would be saved
        raise RuntimeError("WORLD_SIZE > 1 needs the fused step (PICONS_FUSED=1): the autograd path does no gradient all-reduce")
    if fused:
        # the largest minibatch the two loaders can produce (an odd --bs gives bs // 2 + bs // 2); shorter ones run on plans of their own
        engine = pstep.StepEngine(args, bs=2 * (args.bs // 2), hw=hw, num_classes=NUM_CLASSES, jhmdb=(DATASET == "jhmdb"), state=model.state_dict(),
                                  device="cuda:%d" % local)
        reducer = engine.make_reducer() if world > 1 else None
        val_engine = engine.val_engine(args.bs)           # validates the step engine's own weights (validation batches hold args.bs clips)
    save_path = os.path.join('train_log_wts', args.exp_id)
    model_save_dir = os.path.join(save_path, time.strftime('%m-%d-%H-%M'))
    prev_best_val_loss = prev_best_train_loss = 10000
    prev_val_path = prev_train_path = None
    first_epoch = 1
    if resumed is not None:
        restore_train_state(resumed, model, optimizer, scheduler, engine, reducer)
        b = resumed["best"]
        prev_best_val_loss, prev_best_train_loss, prev_val_path, prev_train_path = b["val_loss"], b["train_loss"], b["val_path"], b["train_path"]
        model_save_dir = b["save_dir"]                 # the run goes on where it started: delete-previous-best keeps working
        first_epoch = resumed["epoch"] + 1
        print("resumed %s: epoch %d finished, lr %g, continuing in %s" % (resume_path, resumed["epoch"], optimizer.param_groups[0]['lr'], model_save_dir))
    os.makedirs(model_save_dir, exist_ok=True)
    if resumed is not None:
        trainstate.set_rng_state(resumed["rng"], rank)
    for e in range(first_epoch, args.epochs + 1):
        train_loss = train(args, model, labeled_loader, unlabeled_loader, optimizer, e, save_path, None, ramp_wt, engine, reducer)
        if engine is not None:
            model.load_state_dict(engine.state_dict())           # the checkpoints below are written from `model`
        val_loss = validate(model, val_loader, e, val_engine)
        # data parallel: every rank must take the same scheduler / checkpoint decisions, so they are taken on the mean of the
        # per-rank losses (each rank saw its own shard); otherwise ReduceLROnPlateau fires on one rank and the replicas
        # train at different learning rates from then on
        train_loss, val_loss = pdist.mean_over_ranks([train_loss, val_loss], device="cuda:%d" % local)
        if rank == 0 and val_loss < prev_best_val_loss:           # checkpoint policy of main_ucf101.py:439-455
            print("validation loss improved: %.4f -> %.4f, checkpoint written" % (prev_best_val_loss, val_loss))
            p = os.path.join(model_save_dir, f'best_model_val_loss_{e}.pth')
            torch.save(model.state_dict(), p)
            prev_best_val_loss = val_loss
            if prev_val_path and e < 20:
                os.remove(prev_val_path)
            prev_val_path = p
        if rank == 0 and train_loss < prev_best_train_loss:
            print("training loss improved: %.4f -> %.4f, checkpoint written" % (prev_best_train_loss, train_loss))
            p = os.path.join(model_save_dir, f'best_model_train_loss_{e}.pth')
            torch.save(model.state_dict(), p)
            prev_best_train_loss = train_loss
            if prev_train_path and e < 20:
                os.remove(prev_train_path)
            prev_train_path = p
        scheduler.step(train_loss)
        if state_path:
            write_train_state(state_path, args, meta, rank, e, model, optimizer, scheduler, engine,
                              dict(val_loss=prev_best_val_loss, train_loss=prev_best_train_loss, val_path=_abs(prev_val_path),
                                   train_path=_abs(prev_train_path), save_dir=_abs(model_save_dir)))
        if epochs_this_run > 0 and e - first_epoch + 1 >= epochs_this_run and e < args.epochs:
            print("PICONS_EPOCHS_THIS_RUN=%d: stopping after epoch %d of %d" % (epochs_this_run, e, args.epochs))
            break
    return train_loss


if __name__ == '__main__':
    a = parse_args()
    print(vars(a))
    run(a)
