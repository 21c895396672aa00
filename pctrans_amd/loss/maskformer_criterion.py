"""PCTrans set criterion: point-sampled mask BCE + dice, reference-point L1, query / mask contrast (re-id) losses,
semantic focal loss and discriminative pixel-embedding loss, with deep supervision over the decoder layers.

Mirrors loss/maskformer_criterion.py:118-506 of the reference (`SetCriterion` and its loss_* methods; the helper
functions dice_loss / sigmoid_ce_loss / calculate_uncertainty at :23-116) and loss/loss.py:297-355
(`discriminative_loss`).  `sigmoid_focal_loss` is fvcore's published formula (the reference imports
fvcore.nn.sigmoid_focal_loss_jit, :21).  The world-size normaliser of `num_masks` uses torch.distributed directly
(all_reduce over RCCL / gloo) instead of detectron2.utils.comm.
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from .. import embedding_loss as _embedding_loss
from .. import point_loss as _point_loss
from .. import reid_query as _reid_query
from .. import targets as _targets
from .point_features import get_uncertain_point_coords_with_randomness, point_sample


def dice_loss(inputs, targets, num_masks: float):
    inputs = inputs.sigmoid().flatten(1)
    numerator = 2 * (inputs * targets).sum(-1)
    denominator = inputs.sum(-1) + targets.sum(-1)
    return (1 - (numerator + 1) / (denominator + 1)).sum() / num_masks


def sigmoid_ce_loss(inputs, targets, num_masks: float):
    return F.binary_cross_entropy_with_logits(inputs, targets, reduction="none").mean(1).sum() / num_masks


def calculate_uncertainty(logits):
    assert logits.shape[1] == 1
    return -(torch.abs(logits))


def sigmoid_focal_loss(inputs, targets, alpha: float = -1, gamma: float = 2, reduction: str = "none"):
    p = torch.sigmoid(inputs)
    ce_loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    if reduction == "mean":
        loss = loss.mean()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


DISCRIMINATIVE_DENSE_BUDGET = 64 * 1024 * 1024      # pixels x labels above which discriminative_loss loops over instances


def discriminative_loss(embedding, seg_gt, delta_v=0.5, delta_d=3, alpha=1, beta=1, gama=0.001):
    """Pull pixels to their instance centroid, push centroids apart (loss/loss.py:297-355)."""
    batch_size, embed_dim = embedding.shape[0], embedding.shape[1]
    var_loss = embedding.new_zeros(())
    dist_loss = embedding.new_zeros(())
    reg_loss = embedding.new_zeros(())
    for b in range(batch_size):
        emb_b, gt_b = embedding[b].reshape(embed_dim, -1), seg_gt[b].reshape(-1)
        labels, inv = torch.unique(gt_b, return_inverse=True)                   # ascending: the reference's loop order
        keep = labels != 0
        num_id = int(keep.sum())
        if num_id == 0:
            zero = embedding.sum() * 0
            var_loss, dist_loss, reg_loss = var_loss + zero, dist_loss + zero, reg_loss + zero
            continue
        if emb_b.shape[1] * labels.numel() > DISCRIMINATIVE_DENSE_BUDGET:
            # a crowded, large sample (1024^2 pixels x 1000 instances would need ~4 GB for the membership matrix): the
            # reference's per-instance loop, O(pixels) memory per instance
            cents = []
            for idx in labels[keep]:
                emb_i = emb_b[:, gt_b == idx]
                mean_i = emb_i.mean(dim=1)
                cents.append(mean_i)
                var_loss = var_loss + torch.mean((torch.norm(emb_i - mean_i.reshape(embed_dim, 1), dim=0) - delta_v) ** 2) / num_id
            centroids = torch.stack(cents)
        else:
            # all instances at once: membership as a one-hot [pixels, labels] matrix, so centroids and per-instance means
            # are two small matrix products (deterministic, unlike scatter-adds) instead of ~8 launches per instance
            member = F.one_hot(inv, labels.numel()).to(emb_b.dtype)
            count = member.sum(0)
            mean = (emb_b @ member) / count                                      # [E, labels]
            spread = (torch.norm(emb_b - mean[:, inv], dim=0) - delta_v) ** 2    # [pixels]
            var_loss = var_loss + ((spread @ member) / count)[keep].sum() / num_id
            centroids = mean[:, keep].t()                                        # [num_id, E]
        if num_id > 1:
            d = torch.norm(centroids.reshape(-1, 1, embed_dim) - centroids.reshape(1, -1, embed_dim), dim=2)
            d = d + torch.eye(num_id, dtype=d.dtype, device=d.device) * delta_d
            dist_loss = dist_loss + torch.sum(F.relu(-d + delta_d) ** 2) / (num_id * (num_id - 1)) / 2
        reg_loss = reg_loss + torch.mean(torch.norm(centroids, dim=1))
    return alpha * var_loss / batch_size + beta * dist_loss / batch_size + gama * reg_loss / batch_size


def _pad_masks(masks):
    """Zero-pad a list of [G_i, H_i, W_i] masks to a common [G_i, Hmax, Wmax] (nested_tensor_from_tensor_list)."""
    H = max(m.shape[1] for m in masks)
    W = max(m.shape[2] for m in masks)
    C = max(m.shape[0] for m in masks)
    out = masks[0].new_zeros((len(masks), C, H, W))
    for i, m in enumerate(masks):
        out[i, :m.shape[0], :m.shape[1], :m.shape[2]].copy_(m)
    return out


def _contrast_logsumexp(pred, label):
    """log(1 + sum_{pos p, neg n} exp(s_n - s_p)) as the reference builds it (:313-327, :347-361)."""
    pos_inds, neg_inds = label == 1, label == 0
    pred_pos = pred * pos_inds.float()
    pred_neg = pred * neg_inds.float()
    pred_pos = pred_pos.masked_fill(neg_inds, float("inf"))
    pred_neg = pred_neg.masked_fill(pos_inds, float("-inf"))
    n = pred.shape[1]
    x = F.pad(pred_neg.repeat(1, n) - torch.repeat_interleave(pred_pos, n, dim=1), (0, 1), "constant", 0)
    return torch.logsumexp(x, dim=1)


def _contrast_softplus(scores, n_pos):
    """The same loss for a batch of items whose first n_pos[i] columns are the positives: the double sum factorises,
    log(1 + sum_n e^{s_n} * sum_p e^{-s_p}) = softplus(logsumexp_neg(s) + logsumexp_pos(-s)).  scores [I, K] -> [I].
    (An item without negatives gives logsumexp over nothing = -inf and a loss of 0, like the reference's lone padded 0.)"""
    pos = torch.arange(scores.shape[1], device=scores.device)[None, :] < n_pos[:, None]
    lse_neg = torch.logsumexp(scores.masked_fill(pos, float("-inf")), dim=1)
    lse_pos = torch.logsumexp((-scores).masked_fill(~pos, float("-inf")), dim=1)
    return F.softplus(lse_neg + lse_pos)


class SetCriterion(nn.Module):
    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio,
                 importance_sample_ratio):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.num_points = num_points
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        # "torch": loss_masks as the reference writes it.  "hip": the point-sampled losses on the device kernels of
        # pctrans_amd/point_loss.py where their conditions hold (CUDA fp32 predictions, target masks of one size, covered
        # geometry), the code below otherwise.  A plain attribute; process default from PCT_POINT_LOSS
        self.point_loss = _point_loss.default()
        # acts only inside the "hip" loss path.  "torch": the candidates' logits from the gather, torch.topk, gather, cat.
        # "hip": one selection kernel instead (point_loss.select_uncertain_points), where it covers the shape.  A plain
        # attribute; process default from PCT_POINT_SELECT
        self.point_select = _point_loss.select_default()
        # "torch": loss_embedding as written below.  "hip": the label map and the loss on the device kernels of
        # pctrans_amd/embedding_loss.py where their conditions hold (device tensors, target masks of one size, fp32 contiguous
        # embedding -- a channels-last one is copied --, covered geometry), the code below otherwise.  A plain attribute; process default from PCT_EMB_LOSS
        self.emb_loss = _embedding_loss.default()
        # "each": loss_masks head by head, as the loops of forward reach them.  "batched": where every head meets the conditions
        # of the "hip" loss path, the selection, the loss and its backward of ALL heads run as one launch each before the loops
        # (point_loss.*_many), with the random numbers the per-head calls would draw; anything else runs head by head.  A plain
        # attribute; process default from PCT_LOSS_HEADS
        self.loss_heads = _point_loss.heads_default()
        # "torch": loss_reid_query / loss_reid_mask reduce their items with _contrast_softplus.  "hip": where the items carry
        # their rows [I, Q] from the device paths (query_contrast: reid_query / reid_dice = "hip"), one launch per loss gives every
        # item's loss and its coefficients (pctrans_amd/reid_query.py: contrast_loss_rows); the code below otherwise.  A plain
        # attribute; process default from PCT_CONTRAST_LOSS
        self.contrast_loss = _reid_query.contrast_default()
        self._target_planes = None
        self._emb_plane_index = None

    def _hip_target_planes(self, targets, like):
        """The images' target masks as one fp32 [sum G, Ht, Wt] tensor and each image's first plane, or None when the masks
        differ in size.  Kept for the calls that follow with the same masks (the ten predictions of a step).  A list that carries
        its planes (targets.TargetList from the device path) hands them over: nothing is concatenated or converted."""
        masks = [t["masks"] for t in targets]
        if not masks or len({tuple(m.shape[-2:]) for m in masks}) != 1 or any(m.dim() != 3 or m.device != like.device for m in masks):
            return None
        key = tuple((m.data_ptr(), m._version, tuple(m.shape), m.dtype) for m in masks)
        if self._target_planes is None or self._target_planes[0] != key:
            planes = _targets.handed_planes(targets, masks, like)
            if planes is None:
                planes = torch.cat(masks).to(torch.float32).contiguous()
            starts = [0]
            for m in masks[:-1]:
                starts.append(starts[-1] + m.shape[0])
            self._target_planes = (key, planes, starts, masks)            # (the masks: their addresses stay theirs while kept)
        return self._target_planes[1], self._target_planes[2]

    def _loss_masks_hip(self, pred, targets, indices, num_masks):
        """loss_masks on the device kernels: the same torch.rand calls in the same order, the 3 P oversampled logits from the
        gather and torch's topk (or, with point_select = "hip", the selection kernel in their place), then BCE + dice and
        their backward in one kernel each.  None when the conditions do not hold."""
        if not (torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 4 and pred.is_contiguous()):
            return None
        got = self._hip_target_planes(targets, pred)
        if got is None or not _point_loss.loss_supported(pred, got[0]):
            return None
        planes, starts = got
        Q = pred.shape[1]
        src = torch.cat([s.to(pred.device) + b * Q for b, (s, _) in enumerate(indices)])
        tgt = torch.cat([t.to(pred.device) + starts[b] for b, (_, t) in enumerate(indices)])
        K = int(src.shape[0])
        if K == 0:
            return None
        num_sampled = int(self.num_points * self.oversample_ratio)
        num_uncertain = int(self.importance_sample_ratio * self.num_points)
        num_random = self.num_points - num_uncertain
        with torch.no_grad():
            coords = torch.rand(K, num_sampled, 2, device=pred.device)
            if (self.point_select == "hip" and num_uncertain > 0
                    and _point_loss.select_supported(pred, coords, num_uncertain)):
                # the same two torch.rand calls in the same order; the selected candidates come in candidate order
                candidates, coords = coords, torch.empty(K, self.num_points, 2, device=pred.device)
                _point_loss.select_uncertain_points(pred, src, candidates, num_uncertain, out=coords, with_index=False)
                if num_random > 0:
                    coords[:, num_uncertain:] = torch.rand(K, num_random, 2, device=pred.device)
            else:
                logits = _point_loss.point_sample_planes(pred, src, coords, 1)
                idx = torch.topk(calculate_uncertainty(logits[:, None])[:, 0, :], k=num_uncertain, dim=1)[1]
                coords = torch.gather(coords, 1, idx[:, :, None].expand(-1, -1, 2))
                if num_random > 0:
                    coords = torch.cat([coords, torch.rand(K, num_random, 2, device=pred.device)], dim=1)
        loss_mask, loss_dice = _point_loss.point_mask_losses(pred, src, planes, tgt, coords, num_masks)
        return {"loss_mask": loss_mask, "loss_dice": loss_dice}

    def _loss_masks_batched(self, outputs, targets, num_masks):
        """loss_masks of the final prediction and every auxiliary head at once, in the order forward's loops reach them: the
        final prediction with indices_list[-1], then auxiliary head i with indices_list[i].  -> a list of {"loss_mask",
        "loss_dice"}, one per head, or None (and no random number drawn) when a condition of the batched path does not hold."""
        if not ("masks" in self.losses and self.point_loss == "hip" and torch.is_tensor(outputs.get("pred_masks"))):
            return None
        aux = outputs.get("aux_outputs", [])
        if len(outputs["indices_list"]) < len(aux) or not all(torch.is_tensor(a.get("pred_masks")) for a in aux):
            return None
        preds = [outputs["pred_masks"]] + [a["pred_masks"] for a in aux]
        indices = [outputs["indices_list"][-1]] + [outputs["indices_list"][i] for i in range(len(aux))]
        pred = preds[0]
        if not all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 4 and p.is_contiguous() for p in preds):
            return None
        got = self._hip_target_planes(targets, pred)
        if got is None or not _point_loss.loss_many_supported(preds, got[0]):
            return None
        planes, starts = got
        dev, Q = pred.device, pred.shape[1]
        K = sum(int(s.shape[0]) for s, _ in indices[0])
        if K == 0 or any(sum(int(s.shape[0]) for s, _ in ind) != K or len(ind) != len(indices[0]) for ind in indices):
            return None
        num_sampled = int(self.num_points * self.oversample_ratio)
        num_uncertain = int(self.importance_sample_ratio * self.num_points)
        num_random = self.num_points - num_uncertain
        if num_uncertain > 0 and not (self.point_select == "hip" and 0 < num_sampled <= _point_loss.MAX_CANDIDATES
                                      and num_uncertain <= num_sampled):
            return None
        if num_uncertain < 0 or num_random < 0 or num_sampled < 0:
            return None
        heads = len(preds)
        offs = torch.tensor([[b * Q for ind in indices for b, (s, _) in enumerate(ind) for _ in range(int(s.shape[0]))],
                             [starts[b] for ind in indices for b, (_, t) in enumerate(ind) for _ in range(int(t.shape[0]))]],
                            dtype=torch.int64).to(dev, non_blocking=True)
        src = (torch.cat([s.to(dev) for ind in indices for s, _ in ind]) + offs[0]).view(heads, K)
        tgt = (torch.cat([t.to(dev) for ind in indices for _, t in ind]) + offs[1]).view(heads, K)
        with torch.no_grad():
            # per head, in order: torch.rand(K, 3 P, 2) then torch.rand(K, num_random, 2), as the per-head calls draw them
            candidates, fresh = _point_loss.draw_head_coords(heads, K, num_sampled, num_random, dev)
            if num_uncertain > 0:
                coords = torch.empty(heads, K, self.num_points, 2, device=dev)
                _point_loss.select_uncertain_points_many(preds, src, candidates, num_uncertain, out=coords, with_index=False)
                if num_random > 0:
                    coords[:, :, num_uncertain:] = fresh
            else:
                coords = fresh
            del candidates
        loss_mask, loss_dice = _point_loss.point_mask_losses_many(preds, src, planes, tgt, coords, num_masks)
        return [{"loss_mask": loss_mask[h], "loss_dice": loss_dice[h]} for h in range(heads)]

    def loss_masks(self, outputs, targets, indices, num_masks):
        assert "pred_masks" in outputs
        if self.point_loss == "hip":
            got = self._loss_masks_hip(outputs["pred_masks"], targets, indices, num_masks)
            if got is not None:
                return got
        src_idx = self._get_src_permutation_idx(indices)
        tgt_idx = self._get_tgt_permutation_idx(indices)
        src_masks = outputs["pred_masks"][src_idx]
        target_masks = _pad_masks([t["masks"] for t in targets]).to(src_masks)[tgt_idx]
        src_masks, target_masks = src_masks[:, None], target_masks[:, None]
        with torch.no_grad():
            point_coords = get_uncertain_point_coords_with_randomness(
                src_masks, calculate_uncertainty, self.num_points, self.oversample_ratio, self.importance_sample_ratio)
            point_labels = point_sample(target_masks, point_coords, align_corners=False).squeeze(1)
        point_logits = point_sample(src_masks, point_coords, align_corners=False).squeeze(1)
        return {"loss_mask": sigmoid_ce_loss(point_logits, point_labels, num_masks),
                "loss_dice": dice_loss(point_logits, point_labels, num_masks)}

    def _loss_embedding_hip(self, emb, targets, alpha, beta, gama):
        """loss_embedding on the device kernels: the label map from the cached target planes, the loss with L = the largest
        target count.  No host synchronisation.  None when the conditions do not hold.  The pixel decoder hands its maps over
        channels-last (dense, not contiguous): the kernels read [B, E, h, w] planes, so such a map is copied once, inside autograd."""
        counts = [int(t["masks"].shape[0]) for t in targets]
        if (torch.is_tensor(emb) and emb.is_cuda and emb.dtype == torch.float32 and emb.dim() == 4 and not emb.is_contiguous()
                and emb.shape[1] <= _embedding_loss.MAX_CHANNELS):
            emb = emb.contiguous()
        if not counts or len(counts) != emb.shape[0] or not _embedding_loss.supported(emb, max(counts)):
            return None
        got = self._hip_target_planes(targets, emb)
        if got is None:
            return None
        planes, starts = got
        key = self._target_planes[0]
        if self._emb_plane_index is None or self._emb_plane_index[0] != key:
            if getattr(targets, "planes", None) is planes:       # handed over with their index vectors
                vec = (targets.starts, targets.counts)
            else:
                vec = torch.tensor([starts, counts], dtype=torch.int32).to(emb.device, non_blocking=True)
            self._emb_plane_index = (key, vec[0], vec[1])
        labels = _embedding_loss.instance_label_map(planes, self._emb_plane_index[1], self._emb_plane_index[2], emb.shape[2:])
        return {"loss_emb": _embedding_loss.discriminative_loss(emb, labels, max(counts), alpha=alpha, beta=beta, gama=gama)}

    def loss_embedding(self, emb, targets, alpha=1, beta=1, gama=0.001):
        if self.emb_loss == "hip":
            got = self._loss_embedding_hip(emb, targets, alpha, beta, gama)
            if got is not None:
                return got
        gt = []
        for target in targets:
            down = F.interpolate(target["masks"][:, None].to(torch.float), size=[emb.shape[2], emb.shape[3]],
                                 mode="nearest")
            down = torch.cat([down.new_zeros((1, 1, down.shape[-2], down.shape[-1])), down])
            gt.append(torch.argmax((down[:, 0] > 0).to(torch.int16), dim=0))
        return {"loss_emb": discriminative_loss(emb, torch.stack(gt), alpha=alpha, beta=beta, gama=gama)}

    def _contrast_rows_hip(self, bt, temperature):
        """The items' losses [I] from the device reduction, or None: the switch is off, the items carry no rows (they came from
        the torch chain) or the kernel does not cover them."""
        if self.contrast_loss not in ("torch", "hip"):
            raise ValueError("SetCriterion.contrast_loss must be 'torch' or 'hip', got %r" % (self.contrast_loss,))
        if self.contrast_loss != "hip" or not all(k in bt for k in ("rows", "image", "key", "owner")):
            return None
        if not _reid_query.contrast_supported(bt["rows"], bt["image"], bt["key"], bt["owner"]):
            return None
        return _reid_query.contrast_loss_rows(bt["rows"], bt["image"], bt["key"], bt["owner"], temperature)

    def loss_reid_query(self, outputs, targets, indices, num_masks):
        items = outputs["pred_qd_query"]
        if len(items) == 0:
            return {"loss_reid_query": 0, "loss_reid_query_aux": 0}
        bt = getattr(items, "batched", None)
        if bt is not None:                       # all items at once (query_contrast.ContrastItems)
            contras = self._contrast_rows_hip(bt, 2.0)
            if contras is None:
                contras = _contrast_softplus(bt["contrast"] / 2.0, bt["n_pos"])
            contras = contras.sum()
            sq = torch.abs(bt["aux_consin"] - bt["aux_label"]) ** 2
            aux = ((sq[bt["aux_rows"]] * bt["aux_valid"]).sum(1) / bt["aux_count"]).sum()
            return {"loss_reid_query": contras / len(items), "loss_reid_query_aux": aux / len(items)}
        contras, aux = 0, 0
        for it in items:
            contras = contras + _contrast_logsumexp(it["contrast"].permute(1, 0) / 2.0, it["label"].unsqueeze(0))
            aux = aux + (torch.abs(it["aux_consin"].permute(1, 0) - it["aux_label"].unsqueeze(0)) ** 2).mean()
        return {"loss_reid_query": contras.sum() / len(items), "loss_reid_query_aux": aux / len(items)}

    def loss_reid_mask(self, outputs, targets, indices, num_masks):
        items = outputs["pred_qd_mask"]
        if len(items) == 0:
            return {"loss_reid_mask": 0}
        bt = getattr(items, "batched", None)
        if bt is not None:
            contras = self._contrast_rows_hip(bt, 0.5)
            if contras is None:
                contras = _contrast_softplus(bt["contrast"] / 0.5, bt["n_pos"])
            return {"loss_reid_mask": contras.sum() / len(items)}
        contras = 0
        for it in items:
            contras = contras + _contrast_logsumexp(it["contrast"].permute(1, 0) / 0.5, it["label"].unsqueeze(0))
        return {"loss_reid_mask": contras.sum() / len(items)}

    def loss_refpoints(self, outputs, targets, indices, num_masks):
        assert "reference_points" in outputs
        idx = self._get_src_permutation_idx(indices)
        src_points = outputs["reference_points"][idx]
        target_points = torch.cat([t["center_points"][i] for t, (_, i) in zip(targets, indices)], dim=0).flatten(1)
        return {"loss_refpoints": F.l1_loss(src_points, target_points, reduction="none").sum() / num_masks}

    def loss_sem(self, outputs, targets):
        assert "sem_mask" in outputs
        logits_pred = outputs["sem_mask"]
        sem = torch.stack([t["fg_masks"] for t in targets])
        out_stride = 8
        one_hot = sem[:, None, out_stride // 2::out_stride, out_stride // 2::out_stride].float()
        num_pos = (one_hot > 0).sum().float().clamp(min=1.0)
        return {"loss_sem": sigmoid_focal_loss(logits_pred, one_hot, alpha=0.25, gamma=2.0, reduction="sum") / num_pos}

    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        return batch_idx, torch.cat([src for (src, _) in indices])

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        return batch_idx, torch.cat([tgt for (_, tgt) in indices])

    def get_loss(self, loss, outputs, targets, indices, num_masks):
        loss_map = {"masks": self.loss_masks, "reid_query": self.loss_reid_query, "reid_mask": self.loss_reid_mask}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](outputs, targets, indices, num_masks)

    def forward(self, outputs, targets, pixel_embedding=None):
        indices = outputs["indices_list"][-1]
        num_masks = sum(len(t["labels"]) for t in targets)
        num_masks = torch.as_tensor([num_masks], dtype=torch.float, device=next(iter(outputs.values())).device)
        world = 1
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(num_masks)
            world = dist.get_world_size()
        if hasattr(self.matcher, "check"):
            self.matcher.check()               # device-side assignments: infeasible cost matrices surface here
        num_masks = torch.clamp(num_masks / world, min=1).item()

        # loss_heads == "batched": the mask losses of all heads, computed once; the loops below take theirs from here
        batched = self._loss_masks_batched(outputs, targets, num_masks) if self.loss_heads == "batched" else None

        losses = {}
        for loss in self.losses:
            if loss == "embedding":
                losses.update(self.loss_embedding(pixel_embedding, targets))
            elif loss == "refpoints":
                losses.update(self.loss_refpoints(outputs, targets, indices, num_masks))
            elif loss == "sem":
                losses.update(self.loss_sem(outputs, targets))
            elif loss == "masks" and batched is not None:
                losses.update(batched[0])
            else:
                losses.update(self.get_loss(loss, outputs, targets, indices, num_masks))

        if "aux_outputs" in outputs:
            for i, aux_outputs in enumerate(outputs["aux_outputs"]):
                indices = outputs["indices_list"][i]
                for loss in self.losses:
                    if "reid" in loss or loss == "sem":
                        continue
                    if not (loss == "embedding" or loss == "refpoints"):
                        if loss == "masks" and batched is not None:
                            l_dict = batched[1 + i]
                        else:
                            l_dict = self.get_loss(loss, aux_outputs, targets, indices, num_masks)
                        losses.update({k + f"_{i}": v for k, v in l_dict.items()})
                    if i != 0:
                        l_dict = self.loss_refpoints(outputs["aux_reference_points"][i - 1], targets, indices,
                                                     num_masks)
                        losses.update({k + f"_{i}": v for k, v in l_dict.items()})
        return losses
