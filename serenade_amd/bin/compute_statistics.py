#!/usr/bin/env python3
"""`serenade-compute-statistics` on the MI355X: stage 2 of the recipe, the interface of
serenade/bin/compute_statistics.py with the per-utterance sums on the GPU.

    python -m serenade_amd.bin.compute_statistics --rootdir dump/train/raw --config conf.yaml --dumpdir dump/train

Every feature file under --rootdir (`.h5`, or `.npz` where h5py is unavailable) is read through FeatsDataset and
serenade_amd.stats.fit_statistics fits StandardScaler on hubert and logmel and MinMaxScaler on score and loud, one
partial_fit per utterance in file order (compute_statistics.py:121-141); `stats.joblib` is written to --dumpdir (:144),
holding sklearn's objects where sklearn is installed.  As in the reference the config is loaded and nothing of it is
read, and --feat_type is accepted and unused.  --feats-scp is accepted and refused: the reference has no reader behind
it either."""
import argparse
import logging
import os

import yaml

from serenade_amd import stats
from serenade_amd.datasets import FeatsDataset


def build_parser():
    p = argparse.ArgumentParser(description="Fit the feature scalers of a preprocessing dump and write stats.joblib.")
    p.add_argument("--feats-scp", "--scp", default=None, type=str, help="not supported; use --rootdir")
    p.add_argument("--rootdir", type=str, help="directory searched for feature files")
    p.add_argument("--config", type=str, required=True, help="the recipe's yaml configuration")
    p.add_argument("--feat_type", type=str, default="mel", help="accepted for compatibility; unused")
    p.add_argument("--dumpdir", default=None, type=str, required=True, help="directory that receives stats.joblib")
    p.add_argument("--verbose", type=int, default=1, help="0: warnings only, 1: progress, 2: debug")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    level = (logging.WARNING, logging.INFO, logging.DEBUG)[max(0, min(args.verbose, 2))]
    logging.basicConfig(level=level, format="%(asctime)s %(levelname)s %(module)s: %(message)s")
    with open(args.config) as f:
        yaml.safe_load(f)  # must parse; nothing of it is read
    if args.feats_scp is not None or args.rootdir is None:
        raise ValueError("Please specify either --rootdir or --feats-scp.")
    os.makedirs(args.dumpdir, exist_ok=True)
    dataset = FeatsDataset(args.rootdir, return_utt_id=True)
    logging.info(f"{len(dataset)} feature files under {args.rootdir}")

    def utterances():
        for item in dataset:
            logging.debug(item["utt_id"])
            yield item

    scaler = stats.fit_statistics(utterances())
    stats.save_statistics(scaler, os.path.join(args.dumpdir, "stats.joblib"))
    logging.info(f"wrote {os.path.join(args.dumpdir, 'stats.joblib')}")


if __name__ == "__main__":
    main()
