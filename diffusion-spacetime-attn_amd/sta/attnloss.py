"""Attention-layout loss: does object i appear inside disc i — asked of the cross-attention itself, as a training signal for W.

sta.attnmaps reads, per object, the softmax mass the pixels put on the object's name tokens (in the global prompt and in its own
local prompt); the share of that mass inside the object's disc is `in_disc_mass`. Here the same quantity is differentiable: the
energy of a readout is (1 - in-disc share)^2, the kind of attention-layout energy cross-attention layout-guidance methods minimise,
evaluated inside the tracked UNet calls. Its gradient reaches q through sta_xattn_token_maps_bwd (attnmaps.TokenMapsFn) and the
blend weights W through the tracked chain that already exists — no CLIP weights, no VAE decode or backward in the tracked epochs.

  layout_energy    maps, discs, valid -> one energy per image (plain torch, fp32; not the hot path)
  AttnLayoutLoss   collector attached to the transformer blocks of one resolution while a tracked trajectory runs

Per UNet call k: A_k = mean over the call's recording blocks of token_maps_tracked(q), E_k = layout_energy(A_k); the loss of a
trajectory is sum_images mean_k E_k. It is a sum of per-call terms, each a function of its own call's activations only — which is
what lets per-call recomputation (plms._CallRecompute) differentiate E_k together with the re-run call's output.

What is NOT claimed: anything about image quality. The loss is pinned numerically (tests/test_attnloss_*.py); whether lower
energies give better pictures needs real weights.
"""
import torch

from . import attnmaps as _am
from . import ops as _ops
from . import prompt_state as _ps


def layout_energy(maps, disc, valid):
    """maps [I, R, N] (>= 0), disc [I, R, N] 0 / 1, valid [I, R] bool -> [I]: per image the mean over its valid readouts of
    (1 - s)^2 with s = sum_p disc maps / sum_p maps; an image without valid readouts gives exactly 0 (and no gradient)."""
    valid = valid.to(torch.bool)
    disc = disc.to(maps.dtype)
    total = torch.where(valid, maps.sum(-1), torch.ones((), dtype=maps.dtype, device=maps.device))
    share = (maps * disc).sum(-1) / total
    e = torch.where(valid, (1.0 - share) ** 2, torch.zeros((), dtype=maps.dtype, device=maps.device))
    return e.sum(-1) / valid.sum(-1).clamp(min=1).to(maps.dtype)


class _EarlyExit(Exception):
    """Raised by record() right behind the q of the block named in `stop_after`: the rest of that UNet call is not needed
    (sta.guidance catches it; nothing else sets `stop_after`)."""


class AttnLayoutLoss:
    """Collector of the attention-layout loss over one tracked trajectory.

    with loss: every BasicTransformerBlock whose N == resolution^2 hands its q to record() on each call it runs WHILE AUTOGRAD IS
    ENABLED (calls under torch.no_grad() — the kept trajectory, the fixed-weight forward of per-call recomputation — record nothing,
    and the inference branch of the blocks is never touched). Blocks find the collector through their `_attn_loss` attribute (None
    otherwise: one attribute test per ordinary call, as `_attn_capture`). The readouts are AttnCapture's: begin(centres, texts,
    names, n_calls) derives the 2 K rows of attnmaps.token_weights over the prompts with local prompts "a photo of <name>", or
    set_readouts(...) fixes them. A readout counts iff its name tokens were found and it has an object; its disc is the object's
    ops.disc_masks at the recording resolution, with the radius of the prompt announced last (sta.prompt_state.disc_radius_sq: 0.2
    image sides unless a canvas trajectory scales its discs).

    A new UNet call starts when a block records a second time (as AttnCapture recognises it) or when the sampler says so
    (next_call()). value() closes the open call and returns sum_images mean_k E_k over the calls recorded under plain autograd plus
    the detached values of the calls differentiated one at a time (take_call(), per-call recomputation).

    Recompute mode `all`: a side value cannot leave a checkpointed forward, so while a loss is attached and autograd is on a
    recording block runs its _forward directly instead of through its own checkpoint(...) — only the few blocks of one resolution
    keep their activations; every other block recomputes as before.

    `block_filter` (None = every block, today's behaviour): a predicate on a BasicTransformerBlock; only the blocks it accepts are
    attached, the others never see the collector. `stop_after` (None = never): a block behind whose record() the call is abandoned
    with _EarlyExit — for a caller that needs the energy of the blocks up to that one and nothing of the call's output."""

    def __init__(self, unet, resolution=16, tokenize=None, M=77, block_filter=None):
        self.unet, self.resolution, self.tokenize, self.M = unet, int(resolution), tokenize, int(M)
        self.block_filter, self.stop_after = block_filter, None
        self.recording = False
        self._explicit = None
        self._blocks = []
        self._reset()

    def _reset(self):
        self.sel_ctx = self.w = self.objects = self.found = self.centres = None
        self.n_calls, self.calls, self.block_calls = 0, 0, 0
        self._disc = self._valid = self._w_dev = None
        self._seen, self._sum, self._nblk = set(), None, 0
        self._terms, self._taken = [], None

    # -- configuration ------------------------------------------------------------------------------
    def set_readouts(self, sel_ctx, w, objects=None, found=None):
        """Explicit readouts for the following trajectories (see AttnCapture.set_readouts)."""
        self._explicit = (list(sel_ctx), torch.as_tensor(w, dtype=torch.float32), objects, found)

    def begin(self, centres, texts=None, names=None, n_calls=1, disc_required=False):
        """Start a new trajectory of `n_calls` UNet calls (the k over which the per-call energies are averaged).
        disc_required (default False: today's rule): a readout also needs a disc with at least one set pixel at the recording resolution
        in its image — on a canvas an object lies outside most windows, and a window image without a valid readout gives exactly 0 and
        no gradient (layout_energy's rule)."""
        helper = _am.AttnCapture(None, self.resolution, tokenize=self.tokenize, M=self.M)
        helper._explicit = self._explicit
        helper.begin(centres, texts=texts, names=names)                 # the same readouts, objects and refusals as the capture
        self._reset()
        self.centres, self.sel_ctx, self.w, self.objects, self.found = helper.centres, helper.sel_ctx, helper.w, helper.objects, helper.found
        self.n_calls = int(n_calls)
        if self.n_calls < 1:
            raise ValueError("n_calls must be >= 1, got %d" % self.n_calls)
        if self.sel_ctx is None:
            return self                                                  # no objects: nothing to read, the loss is 0
        I, R, res = len(self.centres), len(self.sel_ctx), self.resolution
        disc = torch.zeros((I, R, res * res), dtype=torch.float32)
        valid = torch.zeros((I, R), dtype=torch.bool)
        found = torch.ones((I, R), dtype=torch.bool) if self.found is None else torch.as_tensor(self.found, dtype=torch.bool).reshape(-1, R).expand(I, R)
        for i in range(I):
            masks = _ops.disc_masks(self.centres[i], res, _ps.disc_radius_sq()).float() if self.centres[i] else None
            for r, o in enumerate(self.objects):
                if o >= 0 and masks is not None:
                    disc[i, r] = masks[o]
                    valid[i, r] = bool(found[i, r]) and (not disc_required or bool(masks[o].any()))
        self._disc, self._valid = disc, valid
        return self

    def __enter__(self):
        if self.centres is None:
            raise RuntimeError("AttnLayoutLoss has no readouts yet: call begin(...) before entering it")
        from ldm.modules.attention import BasicTransformerBlock
        self._blocks = [m for m in self.unet.modules() if isinstance(m, BasicTransformerBlock)
                        and (self.block_filter is None or self.block_filter(m))]
        for blk in self._blocks:
            blk._attn_loss = self
        self.recording = True
        return self

    def __exit__(self, *exc):
        self.recording = False
        for blk in self._blocks:
            blk._attn_loss = None
        return False

    # -- what the blocks call -----------------------------------------------------------------------
    def wants(self, n):
        return self.recording and self.sel_ctx is not None and n == self.resolution * self.resolution and torch.is_grad_enabled()

    def record(self, block, q, cache):
        if id(block) in self._seen:
            self.next_call()
        self._seen.add(id(block))
        I = q.shape[0] // 2
        if self._w_dev is None or self._w_dev.device != q.device:       # one host -> device copy per trajectory, not per block call
            self._w_dev = _am._expand_w(self.w, I, len(self.sel_ctx), cache.packed.M, q.device)
            self._disc, self._valid = self._disc.to(q.device), self._valid.to(q.device)
        maps = _am.token_maps_tracked(q, cache.packed, self.sel_ctx, self._w_dev, block.attn2.scale)
        self._sum = maps if self._sum is None else self._sum + maps
        self._nblk += 1
        self.block_calls += 1
        if block is self.stop_after:
            raise _EarlyExit()

    def next_call(self):
        """Close the UNet call being recorded (the sampler announces a new one; a no-op when nothing was recorded since)."""
        if self._sum is None:
            return
        self._terms.append(layout_energy(self._sum / self._nblk, self._disc, self._valid))       # [I]
        self._seen.clear()
        self._sum, self._nblk = None, 0
        self.calls += 1

    # -- the loss -----------------------------------------------------------------------------------
    def take_call(self):
        """Per-call recomputation: close the call the eager re-run just recorded and hand its E_k [I] (an autograd value of that
        re-run alone) to the caller, who differentiates it with the call's output; its detached value stays in value(). None when
        the re-run recorded nothing."""
        self.next_call()
        if not self._terms:
            return None
        term = self._terms.pop()
        part = term.detach().sum() / self.n_calls
        self._taken = part if self._taken is None else self._taken + part
        return term

    def graph_value(self):
        """sum_images mean_k E_k over the calls recorded under plain autograd so far (an autograd value), or None if there are none."""
        self.next_call()
        if not self._terms:
            return None
        return torch.stack(self._terms).sum() / self.n_calls

    def value(self):
        """The whole loss as a detached scalar tensor: the plain-autograd calls plus every call handed out by take_call()."""
        g = self.graph_value()
        parts = [p for p in (None if g is None else g.detach(), self._taken) if p is not None]
        return sum(parts) if parts else torch.zeros(())
