"""vqnerf_release_amd -- MI355X-native (gfx950) implementation of the VQ-NeRF hot path.

Layout (only what the hot path needs):
    csrc/        hand-written HIP kernels + the C ABI declared in include/: vqnerf_hip.h and one header per later area
                 (vqn_neus_fold.h, vqn_mesh.h, vqn_eval.h, vqn_material_edit.h, vqn_image_codec.h)
    lib/         the built libvqnerf_hip.so (git-ignored, travels to the GPU box)
    _C.py        ctypes binding of that C ABI (fails loudly when the library is missing)
    geo/         host-side mirror of geo/NeuS-ours2/models/{renderer,fields,embedder}.py
    decomp/      host-side mirror of decomp/nerfvq_nfr3/nerfactor/{networks,models,util}
"""
__version__ = '0.1.0'


# ---- weights epoch -------------------------------------------------------------------------------------------------------
# The inference paths keep the networks' parameters re-laid as MFMA fragments ("packs") and rebuild a pack when a parameter
# changes.  torch's per-tensor `_version` counter does NOT see every write: the fused / capturable Adam
# (`torch._fused_adam_`) leaves it untouched, so does a replayed HIP graph, so does any raw-pointer writer behind the C ABI.
# Every pack cache therefore also keys on this process-wide counter.  It advances after every `optimizer.step()` of any torch
# optimiser (global post-step hook below), after every graph replay of the package's trainers, and on request.
# A second counter, the REWRITE epoch, advances on request only (`weights_changed()`, `parallel.broadcast_module`): packs of
# FROZEN parameters -- moved by no optimiser and no replay -- key on it instead, so that a training step of the other nets does
# not rebuild them (a rebuild reads biases back to the host, which a captured step cannot record).
_weights_epoch = [0]
_rewrite_epoch = [0]


def weights_epoch():
    return _weights_epoch[0]


def rewrite_epoch():
    return _rewrite_epoch[0]


def weights_changed():
    """Invalidate every cached weight pack / codebook-fragment image of the process, frozen parameters' included.  Call it after
    rewriting parameters in a way torch cannot see (replaying a captured graph of your own, a ctypes kernel or DLPack peer writing
    into a parameter, `p.data.copy_`)."""
    _weights_epoch[0] += 1
    _rewrite_epoch[0] += 1


def weights_stepped():
    """An optimiser step or a graph replay of a training step moved the TRAINABLE parameters: invalidate the packs keyed on them
    (not those of frozen parameters)."""
    _weights_epoch[0] += 1


class WeightsStamp:
    """What a weight-derived cache was built from: the tensor objects themselves (held weakly: the `id()` or `data_ptr()` of a
    freed tensor is recycled by the next one), their `_version`s and devices, and `extra` (the epochs).  Equal stamps: same
    objects, alive, same versions, same extra."""
    __slots__ = ('refs', 'key')
    __hash__ = None

    def __init__(self, tensors, extra=()):
        import weakref
        self.refs = tuple(weakref.ref(t) for t in tensors)
        self.key = tuple(extra) + tuple((t._version, str(t.device)) for t in tensors)

    def __eq__(self, other):
        return (isinstance(other, WeightsStamp) and self.key == other.key and len(self.refs) == len(other.refs)
                and all(a() is not None and a() is b() for a, b in zip(self.refs, other.refs)))

    def __reduce__(self):                 # a copied / pickled cache matches nothing: it rebuilds on first use
        return WeightsStamp, ((), ('copied',))


def _install_optimizer_hook():
    try:
        from torch.optim.optimizer import register_optimizer_step_post_hook
        register_optimizer_step_post_hook(lambda *_a, **_k: weights_stepped())
    except Exception:                     # noqa: BLE001  (an older torch: trainers of this package still call weights_stepped())
        pass


_install_optimizer_hook()
