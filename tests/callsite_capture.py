"""Record what the head's HIP entry points receive and return at their real call sites (a plain helper module, like
msda_cases.py).  `CallsiteCapture(select).install(monkeypatch)` wraps the product entry points at the module attributes
the call sites look up; every top-level call is recorded as a `Call`: its arguments by name (tensors cloned, modules kept
by reference), its output, and for the MSDeformAttn entries the kernel family the library launched.  A wrapped entry point
that calls another one (a fallback) is recorded once, as the outer call.

`select`: image indices to keep (None = all).  The batch axis follows the call site's layout: encoder token rows and NCHW
maps are image-major (axis 0), the decoder's attention operands are [tokens, N, C] (axis 1), its masks [N, ...].

`entries`: the entry points to wrap (default: the head's forward, ENTRY_POINTS).  A training step adds TRAINING_ENTRIES:
the MSDeformAttn backward (called from autograd's device thread, so the re-entry depth is per thread; its record carries
the backward family) and the batched assignment of the matcher."""
import functools
import inspect
import threading

import torch

# entry point -> {argument name: batch axis}; "out" is the entry's result (a tensor, a list or a tuple of tensors)
LAYOUTS = {
    "fused_ops.linear": {"x": 0, "x_add": 0, "out": 0},
    "fused_ops.linear_k128_multi": {"x": 0, "x_add": 0, "out": 0},
    "fused_ops.linear_add_layer_norm": {"x": 0, "residual": 0, "out": 0},
    "fused_ops.linear_layer_norm": {"x": 0, "residual": 0, "out": 0},
    "fused_ops.ffn_layer_norm": {"x": 0, "out": 0},
    "fused_ops.conv1x1_nchw": {"x": 0, "out": 0},
    "fused_ops.conv1x1_groupnorm_tokens_into": {"x": 0, "out": 0},
    "fused_ops.groupnorm_flatten_into": {"x": 0, "out": 0},
    "fused_ops.conv1x1_from_token_rows": {"x": 0, "out": 0},
    "fused_ops.masked_attention": {"q": 1, "k": 1, "v": 1, "attn_mask": 0, "v_t": 0, "out": 1},
    "fused_ops.cross_attention": {"q_content": 1, "q_pos": 1, "k_content": 1, "k_pos": 1, "v": 1, "attn_mask": 0,
                                  "row_open": 0, "out": 1},
    "MSDA.ms_deform_attn_fused_forward": {"value": 0, "reference_points": 0, "sampling_offsets": 0,
                                          "attention_logits": 0, "out": 0},
    "MSDA.ms_deform_attn_forward": {"value": 0, "sampling_loc": 0, "attn_weight": 0, "out": 0},
    "dynamic_mask_head.dynamic_mask_head_forward": {"mask_feats": 0, "ref_xy": 0, "params": 0, "feats_f32": 0,
                                                    "out": 0},
}
ENTRY_POINTS = tuple(LAYOUTS)
MSDA_ENTRIES = ("MSDA.ms_deform_attn_fused_forward", "MSDA.ms_deform_attn_forward")

# the training step's own entry points (looked up as module attributes by MSDeformAttnFunction.backward and
# Point_HungarianMatcher._assign_padded)
TRAINING_LAYOUTS = {
    "MSDA.ms_deform_attn_backward": {"value": 0, "sampling_loc": 0, "attn_weight": 0, "grad_output": 0, "out": 0},
    "fused_ops.lsap": {"cost": 0, "num_target": 0, "out": 0},
}
TRAINING_ENTRIES = tuple(TRAINING_LAYOUTS)


def _module(prefix):
    import pctrans_amd.dynamic_mask_head as dmh
    from pctrans_amd import MultiScaleDeformableAttention as MSDA
    from pctrans_amd import fused_ops
    return {"fused_ops": fused_ops, "MSDA": MSDA, "dynamic_mask_head": dmh}[prefix]


class Call:
    """One recorded call: `args` {name: value}, `out`, `kernel` (MSDeformAttn forward or backward family id, else None),
    `images` (the original indices of the images kept, None = all)."""

    def __init__(self, entry, args, out, kernel, images):
        self.entry, self.args, self.out, self.kernel, self.images = entry, args, out, kernel, images

    def __repr__(self):
        shapes = {k: tuple(v.shape) for k, v in self.args.items() if torch.is_tensor(v)}
        return "Call(%s, %s)" % (self.entry, shapes)


def _take(t, axis, images):
    """The kept images of `t` along `axis`, cloned; a batch-1 (broadcast) operand is kept whole."""
    if not torch.is_tensor(t):
        return t
    t = t.detach()
    if images is not None and t.dim() > axis and t.shape[axis] != 1:
        t = t.index_select(axis, torch.as_tensor(images, device=t.device))
    elif images is not None and t.dim() > axis and t.stride(axis) == 0:
        t = t.narrow(axis, 0, 1)
    return t.clone()


def _take_any(o, axis, images):
    if isinstance(o, (list, tuple)):
        return type(o)(_take_any(x, axis, images) for x in o)
    return _take(o, axis, images)


class CallsiteCapture:
    def __init__(self, select=None, entries=ENTRY_POINTS):
        self.select = None if select is None else [int(i) for i in select]
        self.calls = {e: [] for e in entries}
        self._local = threading.local()                   # .depth: wrapped calls in progress on this thread

    def install(self, monkeypatch):
        for entry in self.calls:
            prefix, name = entry.split(".")
            mod = _module(prefix)
            monkeypatch.setattr(mod, name, self._wrap(entry, getattr(mod, name)))
        return self

    def counts(self):
        return {e: len(c) for e, c in self.calls.items()}

    def _images(self, batch):
        if self.select is None:
            return None
        return sorted(set(i if i >= 0 else batch + i for i in self.select if -batch <= i < batch))

    def _wrap(self, entry, fn):
        sig = inspect.signature(fn)
        layout = LAYOUTS[entry] if entry in LAYOUTS else TRAINING_LAYOUTS[entry]

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            depth = getattr(self._local, "depth", 0)
            if depth:                                         # a fallback inside another wrapped entry point
                return fn(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = dict(bound.arguments)
            first = next(n for n in layout if n != "out" and torch.is_tensor(args.get(n)))
            images = self._images(args[first].shape[layout[first]])
            rec = {k: (_take(v, layout[k], images) if (k in layout and k != "out" and torch.is_tensor(v)) else v) for k, v in args.items()}
            if torch.is_tensor(args.get("attn_mask")) and args["attn_mask"].dim() == 2:   # [L, S]: shared by the images
                rec["attn_mask"] = args["attn_mask"].detach().clone()
            if entry == "dynamic_mask_head.dynamic_mask_head_forward":
                # the kernel reads these fp32 features (the caller's copy when it hands one over)
                ff = args["feats_f32"] if args["feats_f32"] is not None else args["mask_feats"].detach().float()
                rec["feats_f32"] = _take(ff, 0, images)
            self._local.depth = depth + 1
            try:
                out = fn(*a, **kw)
            finally:
                self._local.depth = depth
            if entry.endswith("_into"):
                # the slice of `out` this call wrote, read after the call; the row offset is in rec["row_offset"]
                h, w = args["x"].shape[2], args["x"].shape[3]
                written = args["out"][:, args["row_offset"]:args["row_offset"] + h * w]
                rec["out"] = None                             # (the whole buffer: other calls write the rest)
                result = _take(written, 0, images)
            else:
                result = _take_any(out, layout["out"], images)
            kernel = None
            if entry in MSDA_ENTRIES:
                from pctrans_amd import _lib
                kernel = int(_lib.lib().pct_msda_last_kernel())
            elif entry == "MSDA.ms_deform_attn_backward":
                from pctrans_amd import _lib
                kernel = int(_lib.lib().pct_msda_last_bwd_kernel())
            self.calls[entry].append(Call(entry, rec, result, kernel, images))
            return out
        return wrapper
