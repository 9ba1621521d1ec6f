"""``python train_Fixmatch_CNN_2D.py --model unet ...`` on MI355X.

Command-line drop-in for the reference's code/train_Fixmatch_CNN_2D.py: same flag names and defaults (:41-68), with
``--patch_size`` taking two ints (``type=list`` there cannot parse a value from a shell).  The hot loop (:247-301) runs as
mis_hip.step.FixMatchTrainer: one network, a forward on the weakly augmented batch (resize + random_rot_flip) and one on
its colour-jittered copy, confidence-masked pseudo labels, the complementary loss under the adaptive sample weight, SGD
with the poly learning rate and the EMA copy the reference maintains.  ``--consistency_type`` and ``--deterministic`` are
parsed and unused, as there.  Snapshots go to ``../model/{exp}_{labeled_num}/{model}`` in the ``util.save_checkpoint`` shape
(train_common.save_checkpoint); ``--load`` resumes from the newest ``model_iter_*.pth`` there.
"""
import argparse

import torch

parser = argparse.ArgumentParser()
parser.add_argument("--root_path", type=str, default="../data/ACDC", help="Name of Experiment")
parser.add_argument("--exp", type=str, default="ACDC/FixMatch_standard_augs", help="experiment_name")
parser.add_argument("--model", type=str, default="unet", help="model_name")
parser.add_argument("--max_iterations", type=int, default=30000, help="maximum epoch number to train")
parser.add_argument("--batch_size", type=int, default=24, help="batch_size per gpu")
parser.add_argument("--deterministic", type=int, default=1, help="whether use deterministic training")
parser.add_argument("--base_lr", type=float, default=0.01, help="segmentation network learning rate")
parser.add_argument("--patch_size", type=int, nargs=2, default=[256, 256], help="patch size of network input")
parser.add_argument("--seed", type=int, default=1337, help="random seed")
parser.add_argument("--num_classes", type=int, default=4, help="output channel of network")
parser.add_argument("--load", default=False, action="store_true", help="restore previous checkpoint")
parser.add_argument("--conf_thresh", type=float, default=0.8, help="confidence threshold for using pseudo-labels")
# label and unlabel
parser.add_argument("--labeled_bs", type=int, default=12, help="labeled_batch_size per gpu")
parser.add_argument("--labeled_num", type=int, default=14, help="labeled data")
# costs
parser.add_argument("--ema_decay", type=float, default=0.99, help="ema_decay")
parser.add_argument("--consistency_type", type=str, default="mse", help="consistency_type")
parser.add_argument("--consistency", type=float, default=0.1, help="consistency")
parser.add_argument("--consistency_rampup", type=float, default=200.0, help="consistency_rampup")


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.step import fixmatch_split
    fixmatch_split(args.batch_size, args.labeled_bs)      # before any device work
    from mis_hip.train_common import run_fixmatch
    from networks.net_factory import net_factory

    def make_model():
        net = net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)
        if net is None:
            raise SystemExit(f"unknown --model {args.model}")
        return net

    return run_fixmatch(args, make_model, label_dtype=torch.uint8)


if __name__ == "__main__":
    print(main())
