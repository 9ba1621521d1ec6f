"""``python train_Contrastive_Cross_CNN_2D.py --model unet ...`` on MI355X.

Command-line drop-in for the reference's code/train_Contrastive_Cross_CNN_2D.py: same flag names and defaults (:32-92),
with ``--patch_size`` taking two ints (``type=list`` there cannot parse a value from a shell).  Two ``net_factory(--model)``
students, the four frozen heads ``net_factory("classifier" | "projector")`` (:135-142), and the loop body (:212-283) as
mis_hip.step.ContrastiveCrossTrainer: cross teaching through Dice on each other's pseudo labels plus the two pixel-wise
contrastive terms, the script's epoch-based consistency ramp and its own learning-rate rule.  Batches come from the weak
(resize-only) loader; the reference's second, strongly augmented loader feeds nothing the loss reads and is not built.
The Swin flags (--cfg, --opts, --zip, --cache-mode, --resume, --accumulation-steps, --use-checkpoint, --amp-opt-level,
--tag, --eval, --throughput), ``--ema_decay``, ``--consistency_type`` and ``--deterministic`` are parsed and unused here,
as there.  Snapshots go to ``../model/{exp}_{labeled_num}_labeled/{model}`` under the reference's file names.
"""
import argparse

parser = argparse.ArgumentParser()
parser.add_argument('--root_path', type=str, default='../data/ACDC', help='Name of Experiment')
parser.add_argument('--exp', type=str, default='ACDC/Cross_teaching_min_max', help='experiment_name')
parser.add_argument('--model', type=str, default='unet', help='model_name')
parser.add_argument('--max_iterations', type=int, default=30000, help='maximum iteration number to train')
parser.add_argument('--batch_size', type=int, default=24, help='batch_size per gpu')
parser.add_argument('--deterministic', type=int, default=1, help='whether use deterministic training')
parser.add_argument('--base_lr', type=float, default=0.01, help='segmentation network learning rate')
parser.add_argument('--patch_size', type=int, nargs=2, default=[224, 224], help='patch size of network input')
parser.add_argument('--seed', type=int, default=1337, help='random seed')
parser.add_argument('--num_classes', type=int, default=4, help='output channel of network')
# label and unlabel
parser.add_argument('--labeled_bs', type=int, default=12, help='labeled_batch_size per epoch')
parser.add_argument('--labeled_num', type=int, default=14, help='labeled data')
# costs
parser.add_argument('--ema_decay', type=float, default=0.99, help='ema_decay')
parser.add_argument('--consistency_type', type=str, default="mse", help='consistency_type')
parser.add_argument('--consistency', type=float, default=0.1, help='consistency')
parser.add_argument('--consistency_rampup', type=float, default=200.0, help='consistency_rampup')
parser.add_argument('--cfg', type=str, default="../code/configs/swin_tiny_patch4_window7_224_lite.yaml",
                    help='path to config file')
parser.add_argument("--opts", help="Modify config options by adding 'KEY VALUE' pairs. ", default=None, nargs='+')
parser.add_argument('--zip', action='store_true', help='use zipped dataset instead of folder dataset')
parser.add_argument('--cache-mode', type=str, default='part', choices=['no', 'full', 'part'])
parser.add_argument('--resume', help='resume from checkpoint')
parser.add_argument('--accumulation-steps', type=int, help="gradient accumulation steps")
parser.add_argument('--use-checkpoint', action='store_true', help="whether to use gradient checkpointing to save memory")
parser.add_argument('--amp-opt-level', type=str, default='O1', choices=['O0', 'O1', 'O2'])
parser.add_argument('--tag', help='tag of experiment')
parser.add_argument('--eval', action='store_true', help='Perform evaluation only')
parser.add_argument('--throughput', action='store_true', help='Test throughput only')


def main(argv=None):
    args = parser.parse_args(argv)
    from mis_hip.step import contrastive_split
    contrastive_split(args.batch_size, args.labeled_bs)      # an odd --labeled_bs is refused before any device work
    from mis_hip.train_common import run_contrastive_cross
    from networks.net_factory import net_factory

    def make_model():
        net = net_factory(net_type=args.model, in_chns=1, class_num=args.num_classes)
        if net is None:
            raise SystemExit(f"unknown --model {args.model}")
        return net

    return run_contrastive_cross(args, make_model, make_model)


if __name__ == "__main__":
    print(main())
