"""Float64 restatements of SetCriterion.loss_refpoints (for all heads at once) and SetCriterion.loss_sem with their gradients, the
known-wrong variants of each, the input families of tests/test_aux_loss_gpu.py and that file's bounds.  Plain helpers on CPU
tensors: tests/test_aux_loss_cpu.py checks the restatements against the criterion in float64 and that every wrong variant leaves
the bounds on these families; the GPU tests compare the kernels with the restatements on the same fp32 operands."""
import torch

U = 2.0 ** -24                      # unit roundoff of fp32


# ---------------------------------------------------------------- reference points
def _pair_ok(s, t, rows, num_targets):
    return 0 <= s < rows and 0 <= t < num_targets


def refpoint_l1(points, target_points, src, tgt, num_masks, shift=0):
    """-> (loss [heads], sum of |terms| / num_masks [heads] -- the same numbers: every term is an absolute value --, the number
    of terms [heads], the number of pairs with an index out of range).  points [heads, rows, dims], target_points [T, dims],
    src / tgt [heads, pairs] integer.  shift: the WRONG pairing -- head h takes the index rows of head h + shift."""
    p, q = points.double(), target_points.double()
    heads, rows, _ = p.shape
    loss = torch.zeros(heads, dtype=torch.float64)
    terms, bad = [0] * heads, 0
    for h in range(heads):
        hh = (h + shift) % heads
        for s, t in zip(src[hh].tolist(), tgt[hh].tolist()):
            if not _pair_ok(s, t, rows, q.shape[0]):
                bad += 1
                continue
            loss[h] += (p[h, s] - q[t]).abs().sum()
            terms[h] += p.shape[2]
    return loss / num_masks, loss / num_masks, terms, bad


def refpoint_l1_grad(points, target_points, src, tgt, num_masks, grad_loss, sign=True):
    """-> (grad_points [heads, rows, dims] float64, the number of pairs that list each row [heads, rows]).  sign=False: the WRONG
    gradient, the difference in place of its sign."""
    p, q = points.double(), target_points.double()
    heads, rows, _ = p.shape
    grad = torch.zeros_like(p)
    count = torch.zeros(heads, rows, dtype=torch.int64)
    for h in range(heads):
        g = float(grad_loss[h]) / num_masks
        for s, t in zip(src[h].tolist(), tgt[h].tolist()):
            if not _pair_ok(s, t, rows, q.shape[0]):
                continue
            d = p[h, s] - q[t]
            grad[h, s] += (torch.sign(d) if sign else d) * g
            count[h, s] += 1
    return grad, count


def refpoint_case(heads, batch, num_query, dims, pairs, seed, empty_image=False, equal=False, repeat=False):
    """fp32 operands of one call: points in (0, 1) like the decoder's sigmoid outputs, pairs distinct rows per head where the rows
    allow it (else drawn with repetition).  empty_image: the last image owns no pair.  equal: the first pair of every head has
    points == target in coordinate 0.  repeat: the second pair of every head lists the first pair's row again."""
    g = torch.Generator().manual_seed(seed)
    rows = batch * num_query
    owned = rows - num_query if empty_image else rows
    num_targets = max(pairs, 1) + 3
    points = torch.rand(heads, rows, dims, generator=g)
    target = torch.rand(num_targets, dims, generator=g)
    src = torch.zeros(heads, pairs, dtype=torch.int64)
    for h in range(heads):
        src[h] = (torch.randperm(owned, generator=g)[:pairs] if pairs <= owned
                  else torch.randint(0, owned, (pairs,), generator=g))
    tgt = torch.randint(0, num_targets, (heads, pairs), generator=g)
    if repeat and pairs >= 2:
        src[:, 1] = src[:, 0]
    if pairs == 1:                               # too few rows for a random draw to tell the heads apart: consecutive heads differ
        src[:, 0] = torch.arange(heads) % owned
        tgt[:, 0] = torch.arange(heads) % num_targets
    if equal and pairs >= 1:
        for h in range(heads):
            points[h, src[h, 0], 0] = target[tgt[h, 0], 0]
    num_masks = float(max(pairs, 1)) + 0.5
    grad_loss = torch.rand(heads, generator=g) + 0.5
    return {"points": points, "target_points": target, "src": src, "tgt": tgt, "num_masks": num_masks, "grad_loss": grad_loss}


# heads 1, 3, 10; batch 1, 2 (an image without pairs); num_query 3, 65, 300; dims 2, 4; pairs 0, 1, 120; an equal coordinate; a
# repeated row; and 1100 pairs on 600 rows: more than one LDS stage of the backward (1024 pairs), more than one pass of the forward
# (256 pairs), more than one workgroup of rows (256), every row listed about twice
REFPOINT_CASES = {
    "h1_b1_q3_d2_p1": dict(heads=1, batch=1, num_query=3, dims=2, pairs=1, seed=1),
    "h3_b2_q65_d4_p120_equal": dict(heads=3, batch=2, num_query=65, dims=4, pairs=120, seed=2, equal=True),
    "h10_b2_q300_d2_p120_empty_repeat": dict(heads=10, batch=2, num_query=300, dims=2, pairs=120, seed=3, empty_image=True,
                                             equal=True, repeat=True),
    "h3_b1_q65_d2_p0": dict(heads=3, batch=1, num_query=65, dims=2, pairs=0, seed=4),
    "h10_b2_q3_d4_p1": dict(heads=10, batch=2, num_query=3, dims=4, pairs=1, seed=5, empty_image=True),
    "h2_b2_q300_d2_p1100": dict(heads=2, batch=2, num_query=300, dims=2, pairs=1100, seed=6),
}


def refpoint_loss_bound(loss64, terms):
    """(n + 2) 2^-24 sum|terms| for n summed terms: one rounding per difference, n - 1 additions, one division; every term is
    non-negative, so sum|terms| / num_masks is the loss itself."""
    return torch.tensor([(n + 2) * U for n in terms], dtype=torch.float64) * loss64.abs()


def refpoint_grad_failures(got, want64, count, grad_loss, num_masks):
    """The gradient rule.  A row no pair lists: exact zeros.  A row one pair lists: the exact sign, and a magnitude within 2 ulp
    of grad_loss / num_masks (an fp32 division, or a product with a reciprocal).  A row c > 1 pairs list: within
    (c + 2) 2^-24 c |g| of the float64 sum (c - 1 additions of terms of magnitude |g|, and g's own rounding)."""
    fails = []
    got = got.double()
    heads = got.shape[0]
    for h in range(heads):
        g = abs(float(grad_loss[h]) / num_masks)
        c = count[h][:, None].expand_as(got[h])
        off = got[h][c == 0]
        if off.numel() and float(off.abs().max()) != 0.0:
            fails.append("head %d: a row without a pair has gradient %g" % (h, float(off.abs().max())))
        one = c == 1
        if bool((torch.sign(got[h][one]) != torch.sign(want64[h][one])).any()):
            fails.append("head %d: a sign differs" % h)
        ulp = 2.0 ** (torch.floor(torch.log2(torch.tensor(g))) - 23) if g > 0 else 0.0
        mag = got[h][one & (want64[h] != 0)].abs()
        if mag.numel() and float((mag - g).abs().max()) > 2 * float(ulp):
            fails.append("head %d: |grad| off grad_loss / num_masks = %.9g by %.3g > 2 ulp" % (h, g, float((mag - g).abs().max())))
        many = c > 1
        if bool(many.any()):
            bound = (c[many] + 2).double() * U * c[many].double() * g
            if bool(((got[h][many] - want64[h][many]).abs() > bound).any()):
                fails.append("head %d: the sum of a repeated row leaves its bound" % h)
    return fails


# ---------------------------------------------------------------- semantic focal loss
def focal_targets(fg, stride, offset=None):
    """fg [N, H, W] -> the float64 targets [N, h, w].  offset: the WRONG first row / column (default stride // 2)."""
    o = stride // 2 if offset is None else offset
    return fg[:, o::stride, o::stride].double()


def sem_focal(logits, fg, stride, alpha, offset=None, use_alpha=True, num_pos_mode="clamped", power=2):
    """-> (loss [], num_pos, per-element terms before the division) in float64.  logits [N, h, w] or [N, 1, h, w].  The keyword
    arguments select the WRONG variants: offset 0, alpha dropped, num_pos "unclamped" or "all" (every pixel counted), power 1."""
    x = logits.double().reshape(logits.shape[0], logits.shape[-2], logits.shape[-1])
    t = focal_targets(fg, stride, offset)
    if t.shape != x.shape:                       # (an offset variant on a map whose slice then has another size)
        t = t[:, :x.shape[1], :x.shape[2]]
    p = torch.sigmoid(x)
    # max(x, 0) - x t + log1p(exp(-|x|)) = (1 - t) x - log sigmoid(x), written so that autograd is right at x = 0 as well (clamp
    # and abs each pick one side there)
    ce = (1 - t) * x - torch.nn.functional.logsigmoid(x)
    m = 1 - (p * t + (1 - p) * (1 - t))
    ell = ce * m ** power
    if alpha >= 0 and use_alpha:
        ell = (alpha * t + (1 - alpha) * (1 - t)) * ell
    if num_pos_mode == "all":
        num_pos = torch.tensor(float(t.numel()), dtype=torch.float64)
    else:
        num_pos = (t > 0).sum().double()
    den = num_pos if num_pos_mode == "unclamped" else num_pos.clamp(min=1.0)
    return ell.sum() / den, num_pos, ell


def sem_focal_grad(logits, fg, stride, alpha, grad_loss=1.0, **variant):
    """d loss / d logits in float64 by autograd of the restatement above (any variant), in the logits' shape."""
    x = logits.double().detach().clone().requires_grad_(True)
    loss = sem_focal(x, fg, stride, alpha, **variant)[0]
    g, = torch.autograd.grad(loss * grad_loss, x)
    return g


def sem_focal_grad_closed(logits, fg, stride, alpha, grad_loss=1.0):
    """The closed form the backward kernel evaluates: grad_loss w ((p - t) m^2 - 2 ce m (2 t - 1) p (1 - p)) / max(num_pos, 1)."""
    x = logits.double().reshape(logits.shape[0], logits.shape[-2], logits.shape[-1])
    t = focal_targets(fg, stride)
    p = torch.sigmoid(x)
    ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    m = 1 - (p * t + (1 - p) * (1 - t))
    w = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)
    num_pos = (t > 0).sum().double().clamp(min=1.0)
    return (grad_loss * w * ((p - t) * m ** 2 - 2 * ce * m * (2 * t - 1) * p * (1 - p)) / num_pos).reshape(logits.shape)


def focal_case(batch, height, width, stride, alpha, fg_dtype, seed, kind="mixed"):
    """fp32 logits [batch, 1, h, w] and the maps fg [batch, height, width] of one call.  The logits are 3 N(0, 1) with the values
    0, +-20 and +-100 planted at the first outputs (both targets where there is room).  The maps are random with about 40 %
    foreground at the sampled pixels, and the pixel stride // 2 rows and columns before each sampled pixel holds the opposite, so
    that a slice from offset 0 sees other targets; kind "background": no sampled pixel is foreground (those other pixels all are);
    kind "fraction" (fp32 maps): some sampled pixels hold 0.5 and 2.0."""
    g = torch.Generator().manual_seed(seed)
    o = stride // 2
    h, w = len(range(o, height, stride)), len(range(o, width, stride))
    logits = 3 * torch.randn(batch, 1, h, w, generator=g)
    t = (torch.rand(batch, h, w, generator=g) < 0.4).float()
    if kind == "background":
        t.zero_()
    flat_x, flat_t = logits.view(-1), t.view(-1)
    special = [0.0, 20.0, -20.0, 100.0, -100.0, 100.0, -100.0, 20.0, -20.0]
    want_t = [1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    for k in range(min(len(special), flat_x.numel())):
        flat_x[k] = special[k]
        if kind != "background":
            flat_t[k] = want_t[k]
    fg = torch.zeros(batch, height, width)
    fg[:, 0::stride, 0::stride][:, :h, :w] = 1 - t          # what a slice from offset 0 would read
    fg[:, o::stride, o::stride] = t
    if kind == "fraction":
        part = fg[:, o::stride, o::stride]
        part[:, ::2, 1::3] = 0.5
        part[:, 1::3, ::2] = 2.0
    return {"logits": logits, "fg": fg.to(fg_dtype), "stride": stride, "alpha": alpha}


# maps 8 x 8 (1 x 1 outputs), 12 x 20, 20 x 28, 512^2 with stride 8; stride 4 once; bool, uint8 and fp32 maps; alpha 0.25 and -1;
# a batch without a positive target; fp32 maps with other values than 0 / 1.  The two largest are for the GPU alone (several
# workgroups: 48 and 256 of them, the second with two passes each)
FOCAL_CASES = {
    "8x8_bool": dict(batch=3, height=8, width=8, stride=8, alpha=0.25, fg_dtype=torch.bool, seed=11),
    "12x20_uint8": dict(batch=2, height=12, width=20, stride=8, alpha=0.25, fg_dtype=torch.uint8, seed=12),
    "20x28_f32": dict(batch=2, height=20, width=28, stride=8, alpha=0.25, fg_dtype=torch.float32, seed=13),
    "20x28_bool_noalpha": dict(batch=2, height=20, width=28, stride=8, alpha=-1.0, fg_dtype=torch.bool, seed=14),
    "20x28_background": dict(batch=2, height=20, width=28, stride=8, alpha=0.25, fg_dtype=torch.bool, seed=15, kind="background"),
    "20x28_fraction": dict(batch=2, height=20, width=28, stride=8, alpha=0.25, fg_dtype=torch.float32, seed=16, kind="fraction"),
    "30x22_stride4": dict(batch=2, height=30, width=22, stride=4, alpha=0.25, fg_dtype=torch.uint8, seed=17),
    "512x512_bool": dict(batch=1, height=512, width=512, stride=8, alpha=0.25, fg_dtype=torch.bool, seed=18),
}
FOCAL_CASES_LARGE = {
    "3x1024x1024_uint8": dict(batch=3, height=1024, width=1024, stride=8, alpha=0.25, fg_dtype=torch.uint8, seed=19),
    "2x1024x1024_stride2": dict(batch=2, height=1024, width=1024, stride=2, alpha=0.25, fg_dtype=torch.bool, seed=20),
}


def torch_chain_sem(logits, fg, stride, alpha, grad_loss=1.0):
    """SetCriterion.loss_sem's chain with this stride and alpha on the operands as they are (fp32 on their device): -> (loss,
    grad_logits).  The yardstick of the project's bound."""
    from pctrans_amd.loss.maskformer_criterion import sigmoid_focal_loss
    x = logits.detach().clone().requires_grad_(True)
    one_hot = fg[:, None, stride // 2::stride, stride // 2::stride].float()
    num_pos = (one_hot > 0).sum().float().clamp(min=1.0)
    loss = sigmoid_focal_loss(x.reshape(one_hot.shape), one_hot, alpha=alpha, gamma=2.0, reduction="sum") / num_pos
    g, = torch.autograd.grad(loss * grad_loss, x)
    return loss.detach(), g


def project_bound(chain, want64):
    """max(2 |torch fp32 chain - f64|, 5e-6 max|f64|), one number for the tensor."""
    return max(2.0 * float((chain.double().cpu() - want64).abs().max()), 5e-6 * float(want64.abs().max()))


# ---------------------------------------------------------------- status codes, no launch
def status_code_failures(L):
    """Argument errors of the four entries on host pointers that are never dereferenced: every call returns before a launch."""
    import ctypes
    BAD, UNSUP, ALIGN = -1, -4, -3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    fails = []

    def expect(what, got, want):
        if got != want:
            fails.append("%s: status %d, expected %d" % (what, got, want))

    fwd, bwd = L.pct_refpoint_l1_forward_f32, L.pct_refpoint_l1_backward_f32
    expect("refpoint forward, 17 heads", fwd(p, p, p, p, 17, 8, 2, 4, 2, 1.0, p, p, None), UNSUP)
    expect("refpoint forward, 9 dims", fwd(p, p, p, p, 2, 8, 9, 4, 2, 1.0, p, p, None), UNSUP)
    expect("refpoint forward, 2^31 rows", fwd(p, p, p, p, 2, 2 ** 31, 2, 4, 2, 1.0, p, p, None), UNSUP)
    expect("refpoint forward, negative pairs", fwd(p, p, p, p, 2, 8, 2, 4, -1, 1.0, p, p, None), BAD)
    expect("refpoint forward, no loss pointer", fwd(p, p, p, p, 2, 8, 2, 4, 2, 1.0, None, p, None), BAD)
    expect("refpoint forward, misaligned src", fwd(p, p, p + 2, p, 2, 8, 2, 4, 2, 1.0, p, p, None), ALIGN)
    expect("refpoint forward, no heads", fwd(p, p, p, p, 0, 8, 2, 4, 2, 1.0, p, p, None), 0)
    expect("refpoint backward, 17 heads", bwd(p, p, p, p, p, 17, 8, 2, 4, 2, 1.0, p, None), UNSUP)
    expect("refpoint backward, 9 dims", bwd(p, p, p, p, p, 2, 8, 9, 4, 2, 1.0, p, None), UNSUP)
    expect("refpoint backward, 2^31 rows", bwd(p, p, p, p, p, 2, 2 ** 31, 2, 4, 2, 1.0, p, None), UNSUP)
    expect("refpoint backward, no grad_loss", bwd(p, p, p, p, None, 2, 8, 2, 4, 2, 1.0, p, None), BAD)
    expect("refpoint backward, no rows", bwd(p, p, p, p, p, 2, 0, 2, 4, 2, 1.0, p, None), 0)
    ffw, fbw = L.pct_sigmoid_focal_strided_forward_f32, L.pct_sigmoid_focal_strided_backward_f32
    expect("focal forward, out_h of offset 0", ffw(p, p, 0, 2, 3, 4, 20, 28, 8, 0.25, p, p, p, None), BAD)
    expect("focal forward, out_w too small", ffw(p, p, 0, 2, 2, 2, 20, 28, 8, 0.25, p, p, p, None), BAD)
    expect("focal forward, map inside the first offset", ffw(p, p, 0, 2, 1, 1, 4, 4, 8, 0.25, p, p, p, None), BAD)
    expect("focal forward, stride 0", ffw(p, p, 0, 2, 2, 3, 20, 28, 0, 0.25, p, p, p, None), BAD)
    expect("focal forward, int32 maps", ffw(p, p, 2, 2, 2, 3, 20, 28, 8, 0.25, p, p, p, None), UNSUP)
    expect("focal forward, 2^31 outputs", ffw(p, p, 0, 32768, 256, 256, 256, 256, 1, 0.25, p, p, p, None), UNSUP)
    expect("focal forward, misaligned workspace", ffw(p, p, 0, 2, 2, 3, 20, 28, 8, 0.25, p + 4, p, p, None), ALIGN)
    expect("focal forward, misaligned fp32 maps", ffw(p, p + 1, 4, 2, 2, 3, 20, 28, 8, 0.25, p, p, p, None), ALIGN)
    expect("focal backward, out_h of offset 0", fbw(p, p, 0, p, p, 2, 3, 4, 20, 28, 8, 0.25, p, None), BAD)
    expect("focal backward, int32 maps", fbw(p, p, 2, p, p, 2, 2, 3, 20, 28, 8, 0.25, p, None), UNSUP)
    expect("focal backward, 2^31 outputs", fbw(p, p, 0, p, p, 32768, 256, 256, 256, 256, 1, 0.25, p, None), UNSUP)
    expect("focal backward, no num_pos", fbw(p, p, 0, None, p, 2, 2, 3, 20, 28, 8, 0.25, p, None), BAD)
    return fails
