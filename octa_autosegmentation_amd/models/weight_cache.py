"""The one staleness rule for packed copies of a parameter (models/mfma_conv.py, models/conv_f32.py): a copy is current while the
invalidation epoch, the parameter's version counter, its storage address and the caller's tag are the ones it was made under.

Optimisers, `load_state_dict` and every in-place op on a parameter move its version counter. Writes through `parameter.data`
(`networks.init_weights`, `dist.broadcast(p.data)`, EMA, checkpoint surgery) move neither the counter nor the storage: call
`invalidate()` after those."""

_EPOCH = [0]


def epoch():
    return _EPOCH[0]


def invalidate():
    """Weights were rewritten behind the version counters: every packed copy made before is stale. Process-wide, not per module tree:
    every other live network repacks once on its next use too (one `octa_pack_conv_weights` launch per network and a few small torch
    kernels per cached layer). For events that happen a handful of times per run (initialisation, checkpoint load, the replicas'
    start-up broadcast); no per-step path calls it."""
    _EPOCH[0] += 1


def cached(weight, slot, tag, make):
    """The value stored ON the parameter object under the attribute `slot` if it was made under the current (epoch, version, storage
    address, tag), else `make()`, stored there. Separate slots do not evict each other (a forward and a data-gradient orientation of
    one weight). Never keyed by id(weight): such a cache served a stale copy when a new parameter was given the id and the storage
    address of a collected one (two DynUNets built one after the other in a test run: logits off by whole units, about one full test
    run in eight); an attribute dies with its parameter."""
    key = (_EPOCH[0], weight._version, weight.data_ptr(), tag)
    hit = getattr(weight, slot, None)
    if hit is None or hit[0] != key:
        hit = (key, make())
        setattr(weight, slot, hit)
    return hit[1]
