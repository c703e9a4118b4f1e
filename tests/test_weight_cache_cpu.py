"""sta.fused.cached_image — the one repack rule of the packed-weight caches ("rebuild this image only when a weight tensor
changed"), on plain CPU tensors with a counting build."""
import torch

from sta import fused


class _Owner:
    pass


def _counting(*weights):
    calls = []

    def build():
        calls.append(1)
        return torch.cat([w.detach().float().reshape(-1) for w in weights]).clone()
    return build, calls


def test_repeated_calls_build_once_and_return_the_image():
    owner, w = _Owner(), torch.arange(6.0).reshape(2, 3)
    build, calls = _counting(w)
    first = fused.cached_image(owner, "a", (w,), build)
    for _ in range(3):
        assert fused.cached_image(owner, "a", (w,), build) is first
    assert len(calls) == 1
    assert torch.equal(first, w.reshape(-1))
    key, value = owner.__dict__["_sta_images"]["a"]
    assert value is first and key == ((w.data_ptr(), w._version, w.dtype),)


def test_in_place_update_rebuilds():
    owner, w = _Owner(), torch.nn.Parameter(torch.ones(4))
    build, calls = _counting(w)
    fused.cached_image(owner, "a", (w,), build)
    with torch.no_grad():
        w.mul_(0.5)
    got = fused.cached_image(owner, "a", (w,), build)
    assert len(calls) == 2 and torch.equal(got, torch.full((4,), 0.5))
    fused.cached_image(owner, "a", (w,), build)
    assert len(calls) == 2


def test_new_storage_rebuilds():
    owner, w = _Owner(), torch.nn.Parameter(torch.ones(4))
    build, calls = _counting(w)
    fused.cached_image(owner, "a", (w,), build)
    keep = w.data                                   # the old storage stays alive: the new one cannot reuse its address
    w.data = torch.full((4,), 3.0)
    got = fused.cached_image(owner, "a", (w,), build)
    assert len(calls) == 2 and torch.equal(got, torch.full((4,), 3.0))
    assert keep.data_ptr() != w.data_ptr()


def test_other_dtype_rebuilds():
    owner = _Owner()
    raw = torch.zeros(8, dtype=torch.float16)
    w16, wb = raw, raw.view(torch.bfloat16)         # same storage, same version counter: only the dtype differs
    assert w16.data_ptr() == wb.data_ptr() and w16._version == wb._version
    calls = []
    fused.cached_image(owner, "a", (w16,), lambda: calls.append(16) or "f16")
    assert fused.cached_image(owner, "a", (wb,), lambda: calls.append(0) or "bf16") == "bf16"
    assert calls == [16, 0]


def test_slots_of_one_owner_are_independent():
    owner, wa, wb = _Owner(), torch.nn.Parameter(torch.ones(2)), torch.nn.Parameter(torch.ones(3))
    (build_a, calls_a), (build_b, calls_b) = _counting(wa), _counting(wb)
    slot_b = ("conv", id(wb))                       # the tuple slots of packed_conv_weight / packed_linear_weight
    a = fused.cached_image(owner, "a", (wa,), build_a)
    b = fused.cached_image(owner, slot_b, (wb,), build_b)
    with torch.no_grad():
        wa.add_(1.0)
    assert fused.cached_image(owner, slot_b, (wb,), build_b) is b
    assert fused.cached_image(owner, "a", (wa,), build_a) is not a
    assert (len(calls_a), len(calls_b)) == (2, 1)
    other = _Owner()                                # ... and another owner has its own images
    fused.cached_image(other, "a", (wa,), build_a)
    assert len(calls_a) == 3 and len(owner.__dict__["_sta_images"]) == 2


def test_two_weights_rebuild_when_either_changes():
    owner, wq, wk = _Owner(), torch.nn.Parameter(torch.ones(2)), torch.nn.Parameter(torch.ones(2))
    build, calls = _counting(wq, wk)
    fused.cached_image(owner, "qk", (wq, wk), build)
    fused.cached_image(owner, "qk", (wq, wk), build)
    assert len(calls) == 1
    with torch.no_grad():
        wk.mul_(2.0)
    assert torch.equal(fused.cached_image(owner, "qk", (wq, wk), build), torch.tensor([1.0, 1.0, 2.0, 2.0]))
    with torch.no_grad():
        wq.mul_(3.0)
    assert torch.equal(fused.cached_image(owner, "qk", (wq, wk), build), torch.tensor([3.0, 3.0, 2.0, 2.0]))
    assert len(calls) == 3


def test_inference_tensor_neither_raises_nor_rebuilds():
    with torch.inference_mode():
        w = torch.ones(4)
    try:
        w._version
    except RuntimeError:
        pass                                        # the case fused._version exists for
    owner = _Owner()
    build, calls = _counting(w)
    first = fused.cached_image(owner, "a", (w,), build)
    assert fused.cached_image(owner, "a", (w,), build) is first
    assert len(calls) == 1
    assert owner.__dict__["_sta_images"]["a"][0] == ((w.data_ptr(), None, w.dtype),)
