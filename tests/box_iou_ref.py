"""The float64 restatement of upstream's box regression loss for BBOX_REG_LOSS_TYPE "giou" / "diou" / "ciou", literal and in plain
torch with autograd: [D2-upstream] FastRCNNOutputLayers.box_reg_loss -> _dense_box_regression_loss (the foreground rows selected by
index, Box2BoxTransform.apply_deltas, the fvcore loss with reduction="sum") divided by max(R, 1), and [fvcore, unverified]
giou_loss / diou_loss / ciou_loss (eps = 1e-7).  Shared by tests/test_box_iou_loss_capi.py and tests/test_gpu_box_iou_loss.py; runs on
whatever device its inputs are on."""
import math

import torch

KINDS = ("giou", "diou", "ciou")
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SCALE_CLAMP = math.log(1000.0 / 16)


def apply_deltas(deltas, boxes, weights=WEIGHTS, scale_clamp=SCALE_CLAMP):
    """[D2-upstream] Box2BoxTransform.apply_deltas, in the dtype of `deltas`."""
    boxes = boxes.to(deltas.dtype)
    widths = boxes[:, 2] - boxes[:, 0]
    heights = boxes[:, 3] - boxes[:, 1]
    ctr_x = boxes[:, 0] + 0.5 * widths
    ctr_y = boxes[:, 1] + 0.5 * heights
    wx, wy, ww, wh = weights
    dx = deltas[:, 0::4] / wx
    dy = deltas[:, 1::4] / wy
    dw = deltas[:, 2::4] / ww
    dh = deltas[:, 3::4] / wh
    dw = torch.clamp(dw, max=scale_clamp)
    dh = torch.clamp(dh, max=scale_clamp)
    pred_ctr_x = dx * widths[:, None] + ctr_x[:, None]
    pred_ctr_y = dy * heights[:, None] + ctr_y[:, None]
    pred_w = torch.exp(dw) * widths[:, None]
    pred_h = torch.exp(dh) * heights[:, None]
    x1 = pred_ctr_x - 0.5 * pred_w
    y1 = pred_ctr_y - 0.5 * pred_h
    x2 = pred_ctr_x + 0.5 * pred_w
    y2 = pred_ctr_y + 0.5 * pred_h
    return torch.stack((x1, y1, x2, y2), dim=-1).reshape(deltas.shape)


def _intersection_and_union(boxes1, boxes2):
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    assert (x2 >= x1).all(), "bad box: x1 larger than x2"
    assert (y2 >= y1).all(), "bad box: y1 larger than y2"
    xkis1 = torch.max(x1, x1g)
    ykis1 = torch.max(y1, y1g)
    xkis2 = torch.min(x2, x2g)
    ykis2 = torch.min(y2, y2g)
    intsct = torch.zeros_like(x1)
    mask = (ykis2 > ykis1) & (xkis2 > xkis1)
    intsct[mask] = (xkis2[mask] - xkis1[mask]) * (ykis2[mask] - ykis1[mask])
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - intsct
    return intsct, union


def giou_loss(boxes1, boxes2, eps=1e-7):
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    intsctk, unionk = _intersection_and_union(boxes1, boxes2)
    iouk = intsctk / (unionk + eps)
    xc1 = torch.min(x1, x1g)
    yc1 = torch.min(y1, y1g)
    xc2 = torch.max(x2, x2g)
    yc2 = torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    miouk = iouk - ((area_c - unionk) / (area_c + eps))
    return (1 - miouk).sum()


def _diou_terms(boxes1, boxes2, eps):
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    intsct, union = _intersection_and_union(boxes1, boxes2)
    union = union + eps
    iou = intsct / union
    xc1 = torch.min(x1, x1g)
    yc1 = torch.min(y1, y1g)
    xc2 = torch.max(x2, x2g)
    yc2 = torch.max(y2, y2g)
    diag_len = ((xc2 - xc1) ** 2) + ((yc2 - yc1) ** 2) + eps
    x_p = (x2 + x1) / 2
    y_p = (y2 + y1) / 2
    x_g = (x1g + x2g) / 2
    y_g = (y1g + y2g) / 2
    distance = ((x_p - x_g) ** 2) + ((y_p - y_g) ** 2)
    return iou, distance, diag_len


def diou_loss(boxes1, boxes2, eps=1e-7):
    iou, distance, diag_len = _diou_terms(boxes1, boxes2, eps)
    return (1 - iou + (distance / diag_len)).sum()


def ciou_loss(boxes1, boxes2, eps=1e-7):
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    iou, distance, diag_len = _diou_terms(boxes1, boxes2, eps)
    w_pred = x2 - x1
    h_pred = y2 - y1
    w_gt = x2g - x1g
    h_gt = y2g - y1g
    v = (4 / (math.pi ** 2)) * torch.pow((torch.atan(w_gt / h_gt) - torch.atan(w_pred / h_pred)), 2)
    with torch.no_grad():
        alpha = v / (1 - iou + v + eps)
    return (1 - iou + (distance / diag_len) + alpha * v).sum()


LOSSES = {"giou": giou_loss, "diou": diou_loss, "ciou": ciou_loss}


def box_reg_loss(kind, proposal_boxes, gt_boxes, pred_deltas, gt_classes, num_classes, weights=WEIGHTS, scale_clamp=SCALE_CLAMP):
    """-> (loss, d loss / d pred_deltas, decoded foreground boxes), all float64, from inputs of any float dtype."""
    pred = pred_deltas.detach().double().requires_grad_(True)
    boxes, gt = proposal_boxes.double(), gt_boxes.double()
    fg_inds = torch.nonzero((gt_classes >= 0) & (gt_classes < num_classes))[:, 0]
    if pred.shape[1] == 4:
        fg_pred_deltas = pred[fg_inds]
    else:
        fg_pred_deltas = pred.view(-1, num_classes, 4)[fg_inds, gt_classes[fg_inds]]
    fg_pred_boxes = apply_deltas(fg_pred_deltas, boxes[fg_inds], weights, scale_clamp)
    loss = LOSSES[kind](fg_pred_boxes, gt[fg_inds]) / max(gt_classes.numel(), 1.0)
    if fg_inds.numel():
        loss.backward()
        grad = pred.grad
    else:
        grad = torch.zeros_like(pred)
    return loss.detach(), grad, fg_pred_boxes.detach()
