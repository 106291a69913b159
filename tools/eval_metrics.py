#!/usr/bin/env python3
"""ldm_exp/test_diffusion.py on the engine: Inception Score, FID, KID and precision / recall of two image folders (searched
recursively), printed as one dict under torch_fidelity's key names.  --input1 is the evaluated set, --input2 the reference set.

The pretrained FID Inception (pt_inception-2015-12-05-6726825d.pth) is not shipped: pass it with --inception-weights (a state dict
with torchvision's key names, as pytorch-fid publishes it).  Without it the network is seeded and the numbers mean nothing beyond
"the pipeline runs".  torch_fidelity's arithmetic is restated from its published definitions, not pinned against it (DESIGN.md
section 6); one GPU.
    python tools/eval_metrics.py --input1 samples/ --input2 imagenet_val/ --inception-weights pt_inception-2015-12-05-6726825d.pth"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--input1', type=str, required=True)
    ap.add_argument('--input2', type=str, required=True)
    ap.add_argument('--inception-weights', type=str, default=None)
    ap.add_argument('--batch-size', type=int, default=50)
    ap.add_argument('--kid-subsets', type=int, default=100)
    ap.add_argument('--kid-subset-size', type=int, default=1000)
    ap.add_argument('--isc-splits', type=int, default=10)
    ap.add_argument('--prc-neighborhood', type=int, default=3)
    args = ap.parse_args(argv)
    M = importlib.import_module('diff-pruning_amd.metrics')
    if not torch.cuda.is_available():
        raise SystemExit('eval_metrics needs an MI355X: there is no CPU path')
    sd = torch.load(args.inception_weights, map_location='cpu') if args.inception_weights else None
    if sd is None:
        print('no --inception-weights: the Inception network is SEEDED, the numbers are not comparable with published ones', file=sys.stderr)
        torch.manual_seed(0)
    model = M.InceptionV3([M.InceptionV3.DEFAULT_BLOCK_INDEX], state_dict=sd).to('cuda')
    metrics_dict = M.calculate_metrics(input1=args.input1, input2=args.input2, isc=True, fid=True, kid=True, prc=True, verbose=False,
                                       samples_find_deep=True, model=model, batch_size=args.batch_size, isc_splits=args.isc_splits,
                                       kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size,
                                       prc_neighborhood=args.prc_neighborhood)
    print(metrics_dict)
    return metrics_dict


if __name__ == '__main__':
    main()
