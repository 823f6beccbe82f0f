#! /usr/bin/env python
"""Reference src/lesion_gnn/scripts/train.py: train from a Python config file. The datasets are
GraphStores saved beforehand (GraphStore.save), one `<dataset name>.pt` per dataset name of the
config, in the directory `--stores`:

    python -m lesion_gnn_amd.scripts.train --config configs/config.py --stores stores/

prints the test metrics as one JSON line."""
from __future__ import annotations

import json
import os
from argparse import ArgumentParser

import torch

from ..datasets import GraphStore
from ..training import train
from ..utils.config import parse_args


def main(argv: list[str] | None = None) -> dict[str, float]:
    parser = ArgumentParser()
    parser.add_argument("--stores", type=str, required=True, metavar="DIR",
                        help="Directory of <dataset name>.pt files written by GraphStore.save.")
    parser.add_argument("--run-dir", type=str, default=None, metavar="DIR",
                        help="Checkpoints and metrics.jsonl "
                             "(default: checkpoints/<project>-seed<seed>).")
    parser.add_argument("--device", type=str, default="cuda")
    args, rest = parser.parse_known_args(argv)
    config = parse_args(rest)
    data = config.dataset
    names = {c.name for c in data.train_datasets + data.val_datasets + data.test_datasets}
    device = torch.device(args.device)
    stores = {name: GraphStore.load(os.path.join(args.stores, f"{name}.pt"), device)
              for name in sorted(names)}
    out = train(config, stores, run_dir=args.run_dir, device=device)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
