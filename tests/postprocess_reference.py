"""Float64 / integer restatement of the device post-processing (include/pctrans_hip_post.h), the reference of
test_postprocess_cpu.py and test_postprocess_gpu.py: the bilinear resize in float64 on exact source coordinates, the threshold
on the logit, the band of pixels too close to the threshold for fp32 to decide, the bit-plane format, the label map from hard
masks, and the decision margins of a case (how far its dice values, cluster means and NMS ratios are from their thresholds and
its areas from one another)."""
import math

import numpy as np
import torch

PARAMS = {"CVPPP": dict(t=0.69, t1=0.5, t2=0.6, hard=True, nms=0.72), "BBBC": dict(t=0.05, t1=0.15, t2=0.25, hard=False, nms=None)}
MIN_AREA = 40


def logit_threshold(dataset):
    """fp32(log(t / (1 - t))), the logarithm in double: a pixel is set where its logit is above this."""
    t = PARAMS[dataset]["t"]
    return float(np.float32(math.log(t / (1.0 - t))))


def _taps(n_in, n_out):
    """Source coordinate of output d: ((2 d + 1) * in - out) / (2 out), clamped at 0 -> (i0, i1, weight of i1) in float64."""
    d = torch.arange(n_out, dtype=torch.int64)
    num = ((2 * d + 1) * n_in - n_out).clamp(min=0)
    i0 = torch.div(num, 2 * n_out, rounding_mode="floor")
    lam = (num - i0 * 2 * n_out).double() / float(2 * n_out)
    return i0, (i0 + 1).clamp(max=n_in - 1), lam


def resize64(logits, size):
    """[..., h, w] -> float64 [..., H, W]: bilinear, align_corners=False; equal sizes are a copy."""
    x = logits.double()
    H, W = int(size[0]), int(size[1])
    h, w = x.shape[-2:]
    if (h, w) == (H, W):
        return x
    y0, y1, ly = _taps(h, H)
    x0, x1, lx = _taps(w, W)
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def threshold64(x64, dataset):
    return x64 > logit_threshold(dataset)


def ambiguous_band(x64, dataset, max_abs_logit):
    """Pixels whose float64 value is within 8 * 2^-24 * max(1, max|logits|) of the threshold: four products and three sums of
    fp32 roundings may put the kernel's value on the other side."""
    return (x64 - logit_threshold(dataset)).abs() <= 8.0 * 2.0 ** -24 * max(1.0, float(max_abs_logit))


def plane_words(H, W):
    return 4 * ((H * W + 127) // 128)


def pack_bits(masks):
    """bool [..., H, W] -> int32 [..., PW], bit (p % 32) of word (p / 32) = pixel p."""
    H, W = masks.shape[-2:]
    pw = plane_words(H, W)
    flat = masks.reshape(masks.shape[:-2] + (H * W,)).to(torch.int64)
    flat = torch.nn.functional.pad(flat, (0, pw * 32 - H * W))
    words = (flat.reshape(flat.shape[:-1] + (pw, 32)) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def unpack_bits(bits, H, W):
    """int32 [..., PW] -> (bool [..., H, W], the padding bits past H*W as bool [..., PW*32 - H*W])."""
    words = bits.to(torch.int64) & 0xFFFFFFFF
    flat = ((words[..., None] >> torch.arange(32, dtype=torch.int64)) & 1).bool().reshape(bits.shape[:-1] + (-1,))
    return flat[..., :H * W].reshape(bits.shape[:-1] + (H, W)), flat[..., H * W:]


def labels_from_masks(masks, dataset):
    """bool [Q, H, W] hard masks at output resolution -> (int16 [H, W] labels, info).  Integers in float64 (exact); the three
    roundings of the reference where it rounds: dice and the cluster mean by fp32 division, the NMS ratio in double.
    info: 'areas' the final masks' areas in label order, 'merged_areas' (CVPPP: the areas NMS orders by), 'margins'."""
    prm = PARAMS[dataset]
    Q, H, W = masks.shape
    flat = masks.reshape(Q, -1).double()
    area = flat.sum(1)
    kept = torch.nonzero(area > MIN_AREA)[:, 0]
    info = dict(areas=[], merged_areas=[], margins=dict(dice=math.inf, mean=math.inf, nms=math.inf))
    if kept.numel() == 0:
        return torch.zeros((H, W), dtype=torch.int16), info
    m, a = flat[kept], area[kept]
    inter = m @ m.t()
    dice = (2 * inter + 1).float() / (a[:, None] + a[None, :] + 1).float()
    info["margins"]["dice"] = float((dice.double() - float(np.float32(prm["t1"]))).abs().min())
    member = dice > float(np.float32(prm["t1"]))
    taken, clusters = set(), []
    for i in range(len(kept)):
        if i in taken:
            continue
        ids = torch.nonzero(member[i])[:, 0].tolist()
        taken.update(ids)
        clusters.append(ids)
    count = torch.stack([m[ids].sum(0) for ids in clusters])                  # [C, HW] integers
    size = torch.tensor([float(len(ids)) for ids in clusters], dtype=torch.float64)
    mean32 = count.float() / size.float()[:, None]
    if prm["hard"]:
        t2 = float(np.float32(prm["t2"]))
        info["margins"]["mean"] = float((mean32.double() - t2).abs().min())
        planes = (mean32 > t2).double()
        areas = planes.sum(1)
        info["merged_areas"] = areas.tolist()
        inter2 = planes @ planes.t()
        order = sorted(range(len(clusters)), key=lambda c: (float(areas[c]), c))[::-1]
        suppressed, keep = [False] * len(clusters), []
        for i, idx in enumerate(order):
            if suppressed[idx]:
                continue
            keep.append(idx)
            for j in order[i:]:
                if suppressed[j]:
                    continue
                aa, bb, ii = float(areas[idx]), float(areas[j]), float(inter2[idx, j])
                if aa == 0 or bb == 0:
                    aa, bb = aa + 0.00001, bb + 0.00001
                ratio = max(ii / aa, ii / bb)
                if j != idx:
                    info["margins"]["nms"] = min(info["margins"]["nms"], abs(ratio - prm["nms"]))
                if ratio >= prm["nms"]:
                    suppressed[j] = True
        final_area = [float(areas[c]) for c in keep]
        values = planes[keep]
    else:
        keep = list(range(len(clusters)))
        final_area = [float(count[c].sum() / size[c]) for c in keep]
        values = mean32.double()
    pos = sorted(range(len(keep)), key=lambda s: (final_area[s], s))
    info["areas"] = [final_area[s] for s in pos]
    scores = torch.cat([torch.zeros((1, H * W), dtype=torch.float64), values[pos]])
    return torch.argmax(scores, dim=0).to(torch.int16).reshape(H, W), info


def instance_labels64(logits, size, dataset):
    """[Q, h, w] logits -> int16 [H, W]: resize64, threshold64, labels_from_masks."""
    return labels_from_masks(threshold64(resize64(logits, size), dataset), dataset)[0]


def areas_distinct(info, dataset):
    """No argsort tie (which torch leaves undefined) decides a label: hard areas all different, soft areas more than 1e-4
    apart relatively."""
    if PARAMS[dataset]["hard"]:
        ok = len(set(info["merged_areas"])) == len(info["merged_areas"])
        return ok and len(set(info["areas"])) == len(info["areas"])
    a = info["areas"]
    return all(b - c > 1e-4 * b for c, b in zip(a, a[1:]))
