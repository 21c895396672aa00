"""The training step's device switches in one table: how each is set, which Python wrappers reach its C entries when every switch
is on, and which torch-side function is the chain it replaces.  Plain helpers (no fixtures): tests/test_train_step_all_on_gpu.py
counts calls through `Watch`, tools/record_train_configs.py sets its configurations through `set_switch`.

A function is named as (owner, attribute[, callers]).  The owner is a module path, a "module.path:Class", or a callable that takes
the model and returns the objects to patch (modules of the model itself).  `callers`, where given, restricts the count to calls
made from those modules: torch.topk and torch.bmm are everybody's.

Per switch:
    wrappers     entered with every switch on, never with every switch off
    torch_side   entered with every switch off, never with every switch on
    superseded   (loss_heads only) the per-head wrappers that its "batched" value replaces: entered in neither of the two, and
                 entered again where the batched path gives way head by head
    count        where the model's structure fixes the number of calls of a step: wrapper label -> function of the model
"""
import importlib
import sys

_PL = "pctrans_amd.point_loss"
_CRIT = "pctrans_amd.loss.maskformer_criterion"
_MATCHER = "pctrans_amd.loss.matcher"
_DEC = "pctrans_amd.transformer_decoder.mask2former_transformer_decoder"
_QC = "pctrans_amd.transformer_decoder.query_contrast"


def _decoder(model):
    return model.sem_seg_head.predictor


def _heads(model):
    """Prediction heads of a step: the query-feature prediction and one per decoder layer."""
    return _decoder(model).num_layers + 1


def _layers(model):
    return _decoder(model).num_layers


def _one(model):
    return 1


def _set_modules(attr):
    def setter(model, value):
        found = [m for m in model.modules() if hasattr(m, attr)]
        assert found, "no module carries the switch %r" % attr
        for m in found:
            setattr(m, attr, value)
    return setter


def _set_point_loss(model, value):
    model.criterion.point_loss = model.criterion.matcher.point_sample = value


def _set_point_select(model, value):
    model.criterion.point_select = value


def _set_match_cost(model, value):
    model.criterion.matcher.match_cost = value


def _set_heads(model, value):
    model.criterion.loss_heads = model.criterion.matcher.cost_heads = value


def _set_emb_loss(model, value):
    model.criterion.emb_loss = value


def _cross_attention_cores(model):
    return [layer.cross_attn for layer in _decoder(model).transformer_cross_attention_layers]


# `flag` / `config_key`: the command-line flag and configuration key of tools/record_train_configs.py.  `set` is None for the
# targets: their mode is an argument of prepare_instance_targets (process default PCT_TARGETS), not an attribute of the model.
SWITCHES = [
    dict(name="dmh_train", flag="--hip-mask-head", config_key="hip_mask_head", set=_set_modules("dmh_train"), on="hip", off="torch",
         wrappers=[("pctrans_amd.dynamic_mask_head", "dynamic_mask_head_backward")],
         torch_side=[(_DEC + ":MultiScaleMaskedTransformerDecoder", "mask_heads_forward_batched")],
         count={"pctrans_amd.dynamic_mask_head:dynamic_mask_head_backward": _heads}),
    dict(name="attn_train", flag="--hip-attn-train", config_key="hip_attn_train", set=_set_modules("attn_train"), on="hip", off="torch",
         wrappers=[("pctrans_amd.attention_train", "cross_attention_forward"), ("pctrans_amd.attention_train", "cross_attention_backward")],
         torch_side=[(_cross_attention_cores, "forward")],
         count={"pctrans_amd.attention_train:cross_attention_forward": _layers,
                "pctrans_amd.attention_train:cross_attention_backward": _layers}),
    dict(name="reid_dice", flag="--hip-reid-dice", config_key="hip_reid_dice", set=_set_modules("reid_dice"), on="hip", off="torch",
         wrappers=[("pctrans_amd.reid_dice", "dice_rows_forward"), ("pctrans_amd.reid_dice", "dice_rows_backward")],
         torch_side=[("torch", "bmm", (_QC,))],
         count={"pctrans_amd.reid_dice:dice_rows_forward": _one, "pctrans_amd.reid_dice:dice_rows_backward": _one}),
    dict(name="point_loss", flag="--hip-point-loss", config_key="hip_point_loss", set=_set_point_loss, on="hip", off="torch",
         wrappers=[(_PL, "point_mask_loss_forward_many"), (_PL, "point_mask_loss_backward")],
         torch_side=[(_CRIT, "get_uncertain_point_coords_with_randomness")],
         count={_PL + ":point_mask_loss_forward_many": _one, _PL + ":point_mask_loss_backward": _one}),
    dict(name="point_select", flag="--hip-point-select", config_key="hip_point_select", set=_set_point_select, on="hip", off="torch",
         wrappers=[(_PL, "select_uncertain_points_many")],
         torch_side=[("torch", "topk", (_CRIT, "pctrans_amd.loss.point_features"))],
         count={_PL + ":select_uncertain_points_many": _one}),
    dict(name="match_cost", flag="--hip-match-cost", config_key="hip_match_cost", set=_set_match_cost, on="hip", off="torch",
         wrappers=[(_PL, "match_costs_many")],
         torch_side=[(_MATCHER, "point_sample")],
         count={_PL + ":match_costs_many": _one}),
    dict(name="loss_heads", flag="--batched-heads", config_key="batched_heads", set=_set_heads, on="batched", off="each",
         wrappers=[(_PL, "point_mask_losses_many"), (_PL, "draw_head_coords")],
         torch_side=[],
         superseded=[(_PL, "point_mask_losses"), (_PL, "select_uncertain_points"), (_PL, "match_costs"), (_PL, "point_sample_planes")],
         count={_PL + ":point_mask_losses_many": _one, _PL + ":draw_head_coords": _one}),
    dict(name="emb_loss", flag="--hip-emb-loss", config_key="hip_emb_loss", set=_set_emb_loss, on="hip", off="torch",
         wrappers=[("pctrans_amd.embedding_loss", "instance_label_map"), ("pctrans_amd.embedding_loss", "discriminative_loss_forward"),
                   ("pctrans_amd.embedding_loss", "discriminative_loss_backward")],
         torch_side=[(_CRIT, "discriminative_loss")],
         count={"pctrans_amd.embedding_loss:instance_label_map": _one, "pctrans_amd.embedding_loss:discriminative_loss_forward": _one,
                "pctrans_amd.embedding_loss:discriminative_loss_backward": _one}),
    # the two C entries (census, planes) are reached from one function; a status word that sends the call back to the torch
    # loop shows as a call of _torch_targets
    dict(name="targets", flag=None, config_key=None, set=None, on="hip", off="torch",
         wrappers=[("pctrans_amd.targets", "_hip_targets")],
         torch_side=[("pctrans_amd.targets", "_torch_targets")],
         count={}),
]


def switch(name):
    return next(s for s in SWITCHES if s["name"] == name)


def set_switch(model, name, on=True):
    s = switch(name)
    s["set"](model, s["on"] if on else s["off"])


def all_on(model):
    """Every training switch of the model at its device value.  (The targets' mode: `targets_mode(True)`.)"""
    for s in SWITCHES:
        if s["set"] is not None:
            s["set"](model, s["on"])
    return model


def all_off(model):
    """Every training switch of the model at the torch chain."""
    for s in SWITCHES:
        if s["set"] is not None:
            s["set"](model, s["off"])
    return model


def targets_mode(on):
    s = switch("targets")
    return s["on"] if on else s["off"]


def label(spec):
    owner = spec[0]
    return "%s:%s" % (owner if isinstance(owner, str) else owner.__name__.strip("_"), spec[1])


def labels(kind, only=None, skip=()):
    """The labels of every function of one kind ("wrappers", "torch_side", "superseded") over the table, or over the switches
    named in `only`, without those named in `skip`."""
    return [label(spec) for s in SWITCHES for spec in s.get(kind, [])
            if (only is None or s["name"] in only) and s["name"] not in skip]


def expected_counts(model, only=None, skip=()):
    """Wrapper label -> calls of one step with every switch on, where the model's structure fixes them."""
    return {k: f(model) for s in SWITCHES for k, f in s["count"].items()
            if (only is None or s["name"] in only) and s["name"] not in skip}


def _owners(spec, model):
    owner = spec[0]
    if not isinstance(owner, str):
        return list(owner(model))
    if ":" in owner:
        mod, cls = owner.split(":")
        return [getattr(importlib.import_module(mod), cls)]
    return [importlib.import_module(owner)]


class Watch:
    """with Watch(model) as w: ... -> w.counts[label]: how often each function of the table was entered.  The functions are
    replaced where their callers look them up (module globals, a class, the model's own sub-modules) and put back on exit."""

    def __init__(self, model):
        self.model = model
        self.counts = {}
        self._undo = []

    def _spy(self, real, key, callers):
        counts = self.counts

        def spy(*args, **kwargs):
            if callers is None or sys._getframe(1).f_globals.get("__name__") in callers:
                counts[key] += 1
            return real(*args, **kwargs)
        return spy

    def __enter__(self):
        for s in SWITCHES:
            for kind in ("wrappers", "torch_side", "superseded"):
                for spec in s.get(kind, []):
                    key = label(spec)
                    self.counts[key] = 0
                    callers = spec[2] if len(spec) > 2 else None
                    for owner in _owners(spec, self.model):
                        had = spec[1] in vars(owner)
                        real = getattr(owner, spec[1])
                        self._undo.append((owner, spec[1], had, vars(owner).get(spec[1])))
                        setattr(owner, spec[1], self._spy(real, key, callers))
        return self

    def __exit__(self, *exc):
        for owner, attr, had, before in reversed(self._undo):
            if had:
                setattr(owner, attr, before)
            else:
                delattr(owner, attr)
        self._undo = []
        return False
