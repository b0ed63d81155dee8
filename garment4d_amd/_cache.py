"""The one packed-weight cache: kernel-layout copies of a module's tensors, kept ON the module in a single plain attribute (a dict of slots: no
buffer, not in state_dict) and rebuilt when a source tensor moves or is written in place.  fused.invalidate() drops that attribute, so a packer
has nothing to register.

Constants that are not a module's (adjacencies, body-model tensors) are cached by object identity in per-site dicts: by_identity()."""
import torch

from . import _lib

ATTR = "_g4d_cache"


def packed(module, slot, tensors, build, extra=None):
    """build() -- run under no_grad -- cached in `slot` of `module`, keyed on (data_ptr, version counter) of `tensors` plus `extra`."""
    key = (tuple((t.data_ptr(), _lib.ver(t)) for t in tensors), extra)
    slots = getattr(module, ATTR, None)
    if slots is None:
        slots = {}
        setattr(module, ATTR, slots)
    hit = slots.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = slots[slot] = (key, build())
    return hit[1]


def drop(root):
    """Forget every slot on `root` and its sub-modules; the number of slots dropped."""
    return sum(len(m.__dict__.pop(ATTR, ())) for m in root.modules())


def by_identity(cache, cap, objs, extra, build):
    """build() cached in the dict `cache` under the identities of the constant objects `objs` plus `extra`.  An entry pins its objects, so their
    ids cannot be recycled while it lives; the dict is emptied once it holds more than `cap` entries."""
    key = (tuple(map(id, objs)), extra)
    hit = cache.get(key)
    if hit is None or not all(a is b for a, b in zip(hit[0], objs)):
        val = build()
        if len(cache) > cap:
            cache.clear()
        hit = cache[key] = (objs, val)
    return hit[1]
