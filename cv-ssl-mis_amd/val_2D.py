"""Validation of a 2-D network on one volume -- drop-in for the reference's code/val_2D.py.

``test_single_volume(image, label, net, classes, patch_size)`` (:18-39): every slice is resized to ``patch_size``
(nearest, scipy ``zoom(order=0)``), run through ``net`` in eval mode, arg-maxed, resized back; per-class
(dice, hd95) of the stacked prediction.  The resizes, the forward and the channel arg-max run on the device
(``mis_augment2d`` gathers, ``mis_argmax_channels`` -- arg-max of the logits == arg-max of their softmax) with one
upload per volume.  ``test_single_volume`` scores on the device too: the label map is uploaded once, the prediction never
leaves the device, and every class is one ``mis_surface_metrics`` call whose 96-byte record gives the very dice / hd95 of
the medpy-free host functions (utils/metrics.py; ``MIS_DEVICE_METRICS=0`` scores with those instead).
"""
import numpy as np
import torch

from mis_hip import ops
from utils import metrics as metric


def calculate_metric_percase(pred, gt):
    pred[pred > 0] = 1
    gt[gt > 0] = 1
    if pred.sum() > 0:
        dice = metric.dc(pred, gt)
        hd95 = metric.hd95(pred, gt) if gt.sum() > 0 else 0   # medpy raises on an empty reference; score it 0
        return dice, hd95
    else:
        return 0, 0


def predict_slices_device(image, net, patch_size, slices_per_launch=16):
    """[Z, X, Y] float image -> [Z, X, Y] uint8 label map on the device.  The volume is uploaded once; both nearest resizes
    (scipy ``zoom(order=0)`` in the reference, :24 and :36) are one ``mis_augment2d`` gather launch over all slices
    (bit-exact to scipy, tests/test_augment_gpu.py), the forward runs on batches of slices."""
    from dataloaders.dataset import zoom_slices
    Z, x, y = image.shape
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            vol = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).cuda()
            inp = zoom_slices(vol, patch_size)                                   # [Z, 1, ph, pw]
            pred = torch.empty((Z, patch_size[0], patch_size[1]), dtype=torch.uint8, device="cuda")
            for z0 in range(0, Z, slices_per_launch):
                logits = net.forward_raw(inp[z0:z0 + slices_per_launch].contiguous(), no_backward=True)   # [n, C, 1, ph, pw]
                ops.argmax_channels(logits, pred[z0:z0 + logits.shape[0]].view(-1))
            back = zoom_slices(pred.float(), (x, y))                             # labels are small integers: exact
            prediction = back[:, 0].to(torch.uint8).contiguous()
    finally:
        net.train(was_training)
    return prediction


def predict_slices(image, net, patch_size, slices_per_launch=16):
    """``predict_slices_device`` with one download: the [Z, X, Y] uint8 label map as a numpy array."""
    return predict_slices_device(image, net, patch_size, slices_per_launch).cpu().numpy()


def device_metric_percase(scores):
    """``calculate_metric_percase`` from a ``utils.metrics.SurfaceScores``: the same rules, decided from the counts."""
    c = scores.counts
    if c["a"] > 0:
        return scores.dc, (scores.hd95 if c["b"] > 0 else 0)
    return 0, 0


def test_single_volume(image, label, net, classes, patch_size=[256, 256]):
    image, label = image.squeeze(0).cpu().detach().numpy(), label.squeeze(0).cpu().detach().numpy()
    gt = metric.device_label_map(label) if metric.device_metrics_enabled() else None
    if gt is None:
        prediction = predict_slices(image, net, patch_size)
        return [calculate_metric_percase(prediction == i, label == i) for i in range(1, classes)]
    prediction = predict_slices_device(image, net, patch_size)
    scores = [metric.device_scores(prediction, gt, i) for i in range(1, classes)]     # all launched before the first read
    return [device_metric_percase(s) for s in scores]
