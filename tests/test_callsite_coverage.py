"""CPU: every compute symbol of the C ABI is either reached through an entry point that tests/callsite_capture.py wraps
(directly, or through that entry point's own fallback) -- so test_callsite_parity_gpu.py checks it at the head's call
sites, or test_callsite_training_gpu.py at a training step's -- or listed below with the reason neither reaches it.  A new
kernel on either path fails here until the capture helper and its float64 reference cover it."""
import dis
import inspect

from callsite_capture import ENTRY_POINTS, TRAINING_ENTRIES, _module

# C ABI symbol -> the wrapped entry point that reaches it on the head's forward path
REACHED = {
    "pct_ms_deform_attn_fused_forward_f32": "MSDA.ms_deform_attn_fused_forward",
    "pct_ms_deform_attn_forward_f32": "MSDA.ms_deform_attn_forward",
    "pct_linear_k128_f32": "fused_ops.linear",
    "pct_linear_k128_multi_f32": "fused_ops.linear_k128_multi",
    "pct_linear_k128_add_layernorm_f32": "fused_ops.linear_add_layer_norm",
    "pct_add_layernorm_f32": "fused_ops.linear_add_layer_norm",          # its fallback below 4 096 token rows
    "pct_linear_add_layernorm_f32": "fused_ops.linear_layer_norm",
    "pct_ffn_layernorm_f32": "fused_ops.ffn_layer_norm",
    "pct_conv1x1_nchw_f32": "fused_ops.conv1x1_nchw",
    "pct_conv1x1_groupnorm_tokens_f32": "fused_ops.conv1x1_groupnorm_tokens_into",
    "pct_groupnorm_flatten_f32": "fused_ops.groupnorm_flatten_into",
    "pct_masked_attention_bf16": "fused_ops.masked_attention",
    "pct_cross_attention_bf16": "fused_ops.cross_attention",
    "pct_dynamic_mask_head_forward": "dynamic_mask_head.dynamic_mask_head_forward",
    "pct_dynamic_mask_head_forward_mfma": "dynamic_mask_head.dynamic_mask_head_forward",
    "pct_dynamic_mask_head_forward_fused_bf16": "dynamic_mask_head.dynamic_mask_head_forward",
}

# C ABI symbol -> the wrapped training entry point that reaches it in a training step (test_callsite_training_gpu.py)
TRAINING_REACHED = {
    "pct_ms_deform_attn_backward_f32": "MSDA.ms_deform_attn_backward",
    "pct_lsap_f32": "fused_ops.lsap",
}

# compute symbols neither the head's forward nor a training step calls
NOT_ON_FORWARD_PATH = {
    "pct_ms_deform_attn_forward_f64": "fp64 values: the reference op's double dispatch, kept for parity; the head is fp32",
    "pct_ms_deform_attn_forward_f16": "16-bit MSDeformAttn values are config 5's path, not the head's (its value is fp32)",
    "pct_ms_deform_attn_forward_bf16": "16-bit MSDeformAttn values are config 5's path, not the head's (its value is fp32)",
    "pct_ms_deform_attn_forward_planes_f32": "the piece-plane operand layout: tests and tools only, no head call site",
    "pct_ms_deform_attn_backward_f64": "fp64 backward: the reference op's double dispatch, kept for parity; training is "
                                       "fp32 (oracle tests in test_msda_gpu)",
}

# not compute: version, errors, build info, pools, diagnostics
SERVICE = {"pct_abi_version", "pct_error_string", "pct_build_info", "pct_prepare_device", "pct_msda_set_kernel_choice",
           "pct_msda_last_kernel", "pct_msda_set_bwd_kernel_choice", "pct_msda_last_bwd_kernel"}


def _symbols_reached_from(fn, seen=None):
    """pct_* names an entry point's code (and that of the same-module functions it calls, transitively) refers to:
    attribute names, and the string values of module-level tables it indexes (MSDA's dtype dispatch)."""
    seen = set() if seen is None else seen
    if fn in seen:
        return set()
    seen.add(fn)
    found = set()
    codes, names, consts = [fn.__code__], set(), set()
    while codes:                                         # the function and the comprehensions / closures inside it
        code = codes.pop()
        codes.extend(c for c in code.co_consts if inspect.iscode(c))
        consts |= {c for c in code.co_consts if isinstance(c, str)}
        names |= set(code.co_names) | {i.argval for i in dis.get_instructions(code) if isinstance(i.argval, str)}
    found |= {n for n in names | consts if n.startswith("pct_")}
    for n in names:
        g = fn.__globals__.get(n)
        if inspect.isfunction(g) and g.__module__ == fn.__module__:
            found |= _symbols_reached_from(g, seen)
        elif isinstance(g, dict):
            found |= {v for v in g.values() if isinstance(v, str) and v.startswith("pct_")}
    return found


def test_every_compute_symbol_is_covered_or_has_a_reason():
    from pctrans_amd import _lib
    compute = set(_lib.SYMBOLS) - SERVICE
    assert SERVICE <= set(_lib.SYMBOLS), sorted(SERVICE - set(_lib.SYMBOLS))
    tables = (set(REACHED), set(TRAINING_REACHED), set(NOT_ON_FORWARD_PATH))
    assert not (tables[0] & tables[1] or tables[0] & tables[2] or tables[1] & tables[2])
    unlisted = compute - set.union(*tables)
    assert not unlisted, "new C ABI compute symbols: wrap their entry point in callsite_capture.py or state why the " \
                         "head never calls them: %s" % sorted(unlisted)
    stale = set.union(*tables) - compute
    assert not stale, "listed but no longer in the ABI: %s" % sorted(stale)
    assert all(reason.strip() for reason in NOT_ON_FORWARD_PATH.values())


def test_reached_symbols_are_called_by_the_wrapped_entry_point_named():
    for sym, entry in list(REACHED.items()) + list(TRAINING_REACHED.items()):
        wrapped = ENTRY_POINTS if sym in REACHED else TRAINING_ENTRIES
        assert entry in wrapped, "%s: %s is not wrapped by callsite_capture" % (sym, entry)
        prefix, name = entry.split(".")
        fn = getattr(_module(prefix), name)
        assert sym in _symbols_reached_from(fn), "%s does not reach %s" % (entry, sym)


def test_every_wrapped_entry_point_reaches_a_listed_symbol():
    """... and nothing a wrapped entry point calls is missing from its table, REACHED or TRAINING_REACHED (unless it is
    listed as not on either path)."""
    for entry in ENTRY_POINTS + TRAINING_ENTRIES:
        prefix, name = entry.split(".")
        syms = _symbols_reached_from(getattr(_module(prefix), name)) - SERVICE
        assert syms, entry
        table = REACHED if entry in ENTRY_POINTS else TRAINING_REACHED
        missing = syms - set(table) - set(NOT_ON_FORWARD_PATH)
        assert not missing, "%s reaches %s, which its table does not list" % (entry, sorted(missing))
