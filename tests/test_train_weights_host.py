"""train_weights._Weights on the CPU (the fragment-order pack kinds build in pure torch there): a cache row belongs
to one pack, so no pack can be left stale by a later grouping of the same parameter."""
import pytest
import torch


def _params(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(32, 32, 3, 3, generator=g)) for _ in range(n)]


def _update(params):
    """what an optimizer step does to the cache's view of the parameters: new values in place, a version bump"""
    with torch.no_grad():
        for p in params:
            p.mul_(-1.5).add_(0.25)  # (in-place ops on a leaf under no_grad bump _version)


def test_second_grouping_of_a_parameter_raises():
    from textmae_amd.train_weights import _Weights

    p, q, r = _params(3)
    W = _Weights(torch.bfloat16)
    pair = W.packed([p, q], "licT")
    with pytest.raises(RuntimeError) as e:
        W.packed([p], "licT")
    # the message names the kind and both groupings
    assert "licT" in str(e.value) and str((id(p),)) in str(e.value) and str((id(p), id(q))) in str(e.value)
    with pytest.raises(RuntimeError):
        W.packed([r, q], "licT")
    assert W.packed([p, q], "licT") is pair          # the same grouping again: the same buffer
    W.packed([p], ("lic", 0, 32))                    # another kind is another row
    with pytest.raises(RuntimeError):
        W.packed([p, q], ("lic", 0, 32))
    W.packed([p, q], ("lic", 8, 16))                 # (other channel range = other kind)
    assert set(W.owner.values()) == set(W.packs)     # every row's owner is a live pack
    assert len(W.owner) == 2 + 1 + 2


def test_every_pack_is_current_after_an_update():
    """the reverse of the stale-pack case (one parameter in a 1-pack and a 2-pack: refresh() walked the rows, which
    the newer pack had taken over, and the older pack kept the old weights): with one pack per row, every pack
    packed() hands out after an in-place update holds the new values"""
    from textmae_amd import ops
    from textmae_amd.train_weights import _Weights

    dt = torch.bfloat16
    p, q, r = _params(3, seed=5)
    W = _Weights(dt)
    asks = [([p, q], "licT"), ([r], "licT"), ([p, q], ("lic", 0, 32)), ([r], ("lic", 8, 16)), ([p], ("lic", 8, 16))]

    def check():
        for params, kind in asks:
            buf = W.packed(params, kind)
            for j, w in enumerate(params):
                ref = (ops.pack_lic_stack_weight_t(w.detach(), dt) if kind == "licT"
                       else ops.pack_lic_stack_weight(w.detach()[:, kind[1]:kind[1] + kind[2]], dt))
                assert torch.equal(buf[j], ref), (kind, j)

    check()
    first = {(tuple(id(w) for w in params), kind): W.packed(params, kind) for params, kind in asks}
    _update([p, q, r])
    assert all(e[0] != (e[2].data_ptr(), e[2]._version) for e in W.cache.values())  # every row is stale now
    check()
    for (ids, kind), buf in first.items():  # re-laid out in place: launches keep their pointers
        assert W.packs[(ids, kind)] is buf


def test_single_entry_is_adopted_by_a_pack():
    """an unpacked single copy asked for before its pack (`conv_dg()` then a "conv_dg" pack): the pack takes the
    row over, and the single lookup returns the pack's row from then on"""
    from textmae_amd.train_weights import _Weights

    p, q = _params(2)
    W = _Weights(torch.float32)
    W.cache[(id(p), "conv_dg")] = [(p.data_ptr(), p._version), torch.empty(32, 288), p, None]  # a built single copy
    W._get = lambda w, kind, make: W.cache[(id(w), kind)][1]  # (no re-layout kernel on the CPU)
    pack = W.packed([p, q], "conv_dg")
    assert W.conv_dg(p).data_ptr() == pack[0].data_ptr() and W.owner[(id(p), "conv_dg")] == ((id(p), id(q)), "conv_dg")
