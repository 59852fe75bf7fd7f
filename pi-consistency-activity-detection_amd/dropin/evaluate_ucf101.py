#!/usr/bin/env python3
"""Drop-in for /root/reference/evaluate_ucf101.py (and, with PICONS_DATASET=jhmdb, evaluate_jhmdb.py): same flags
(`--ckpt`, `--seed`, :28-31), same per-checkpoint loop (`best_model_<split>*.pth`, :48-55), same clip construction,
thresholds, printed line (:79-186) and the same pruning of all but the best f-mAP / v-mAP checkpoints (:190-204) - with
the network on the HIP kernels and the per-frame IoU / per-class accumulation on the device
(picons_amd.evalmetrics, csrc/evalmetrics.hip) instead of numpy on the host.

Environment only (the CLI is unchanged):
  PICONS_SYNTHETIC=1      synthetic videos (the dataset / decoder libraries are not on the box); 0 imports the caller's
                          datasets.ucf_dataloader_eval.UCF101DataLoader from PYTHONPATH
  PICONS_EVAL_VIDEOS=<n>  number of synthetic videos (default 4)
  PICONS_EVAL_PACK=1      clips of consecutive videos share full batches (same tables, ~2x the clips/s on short videos)
  PICONS_EVAL_ENGINE=1    (default 0) the pass runs on picons_amd.evalstep.EvalEngine: videos go up as the decoder left them (uint8 frames and
                          uint8 truth -- the synthetic ones, or with real data the caller's `load_video(...)` instead of `__getitem__`), clips are
                          cut on the device, one plan serves every batch and every checkpoint is loaded into the one engine.  Same printed
                          line, same pruning.  The real-data branch needs skvideo / cv2 / scipy and has not been run where this was written.
  PICONS_KEEP_CKPTS=1     do not delete the checkpoints that are neither best f-mAP nor best v-mAP
  PICONS_DATASET=jhmdb    21 classes (evaluate_jhmdb.py:45)
"""
import argparse
import glob
import os
import os.path as osp
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bootstrap  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch  # noqa: E402

from picons_amd import evalmetrics, synthetic, trainstate  # noqa: E402


def _videos(n_classes, hw=224):
    if os.environ.get("PICONS_SYNTHETIC", "1") == "1":
        return synthetic.make_eval_videos(int(os.environ.get("PICONS_EVAL_VIDEOS", "4")), num_classes=n_classes, hw=hw)
    from datasets.ucf_dataloader_eval import UCF101DataLoader          # the caller's loader (needs skvideo / the dataset)
    ds = UCF101DataLoader('validation', [hw, hw], 1, file_id="testing_annots.pkl", use_random_start_frame=False)
    return (ds[i] for i in range(len(ds)))


def _videos_u8(n_classes, jhmdb, hw):
    """PICONS_EVAL_ENGINE=1: (frames uint8 [F,H,W,3], truth uint8 [F,H,W,1], label) per video, before the centre crop and the division by 255."""
    if os.environ.get("PICONS_SYNTHETIC", "1") == "1":
        yield from synthetic.make_eval_videos_u8(int(os.environ.get("PICONS_EVAL_VIDEOS", "4")), num_classes=n_classes, hw=hw)
        return
    if jhmdb:
        from datasets.jhmdb_dataloader_eval import JHMDB                   # the caller's loaders (need cv2 / scipy / skvideo and the dataset)
        ds = JHMDB('test', [hw, hw], file_id=None)
    else:
        from datasets.ucf_dataloader_eval import UCF101DataLoader
        ds = UCF101DataLoader('validation', [hw, hw], 1, file_id="testing_annots.pkl", use_random_start_frame=False)
    for entry in ds.vid_files:
        got = ds.load_video(*entry) if isinstance(entry, (tuple, list)) else ds.load_video(entry)
        if got[0] is None:
            continue
        frames, truth, label = got[:3]
        yield np.ascontiguousarray(frames, np.uint8), np.ascontiguousarray(truth).astype(np.uint8, copy=False), label


def iou(split, argv=None, hw=224, on_engine=None):
    """Accuracy, f-mAP and v-mAP over the test set for every `best_model_<split>*.pth` under --ckpt.  hw: the crop (the reference's 224; the
    tests run smaller); on_engine(engine): called once with the EvalEngine of PICONS_EVAL_ENGINE=1 before the first checkpoint."""
    parser = argparse.ArgumentParser(description='evaluation')
    parser.add_argument('--ckpt', type=str, help='experiment name')
    parser.add_argument('--seed', type=int, default=47, help='seed for initializing training.')
    args = parser.parse_args(argv)
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)

    synthetic_mode = os.environ.get("PICONS_SYNTHETIC", "1") == "1"      # read only: the process environment is not written to
    jhmdb = os.environ.get("PICONS_DATASET", "ucf101") == "jhmdb"
    n_classes = 21 if jhmdb else 24
    if jhmdb:
        from models.capsules_jhmdb_semi_sup_pa import CapsNet
    else:
        from models.capsules_ucf101 import CapsNet
    # every checkpoint loaded below overwrites the whole state, so in synthetic mode a missing rgb_charades.pt (no network) is passed
    # over EXPLICITLY with pt_path=None; with real data CapsNet() raises for a missing trunk file like the reference does
    pt_path = '../weights/rgb_charades.pt'
    clip_batch_size = 14
    pack = os.environ.get("PICONS_EVAL_PACK", "0") == "1"
    use_engine = os.environ.get("PICONS_EVAL_ENGINE", "0") not in ("", "0")
    if use_engine:
        from picons_amd import evalstep
        model = None
        engine = evalstep.EvalEngine(bs=clip_batch_size, hw=hw, num_classes=n_classes)
        if on_engine is not None:
            on_engine(engine)
    else:
        kw = {} if hw == 224 else {"hw": hw}
        model = (CapsNet(pt_path=None, **kw) if (synthetic_mode and not os.path.exists(pt_path)) else CapsNet(**kw)).cuda()
    model_names, fmap_best, vmap_best, results = [], [], [], []
    files = sorted(glob.glob(osp.join(args.ckpt, 'best_model_' + split + '*.pth')))
    for saved_wts in files:
        model_names.append(saved_wts)
        if use_engine:
            engine.load_state(trainstate.model_state_of(torch.load(saved_wts, map_location="cpu")))
            print('loaded weights from previous run: ', saved_wts)
            r = engine.evaluate(_videos_u8(n_classes, jhmdb, hw), pack=pack)
        else:
            model.load_previous_weights(saved_wts)
            model.eval()
            model.training = False
            r = evalmetrics.evaluate(model, _videos(n_classes, hw), n_classes=n_classes, clip_batch_size=clip_batch_size, pack=pack).result()
        thr = np.arange(0, 20, dtype=np.float32) / 20
        print('Accuracy:', r["accuracy"], 'IoU/fmap/vmap', thr[4], r["fmAP"][4], r["vmAP"][4], thr[10], r["fmAP"][10], r["vmAP"][10])
        fmap_best.append(r["fmAP"][10]); vmap_best.append(r["vmAP"][10]); results.append(r)
    if not files:
        return results
    best = {model_names[fmap_best.index(max(fmap_best))], model_names[vmap_best.index(max(vmap_best))]}
    if os.environ.get("PICONS_KEEP_CKPTS", "0") != "1":
        for f in files:
            if f not in best:
                os.remove(f)
    print(os.listdir(args.ckpt))
    return results


if __name__ == '__main__':
    iou('train')
