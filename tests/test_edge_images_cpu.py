"""CPU: the operand-image cache of the gather-side edge convolutions (spgan.edge_conv.cached_images behind rank_images, upsample_images
and weight_images).  The builders are plain torch and ops.capturing() is false without a capture, so CPU tensors exercise all of it.

Shapes: the smallest at which every slice of every image is non-trivial and no two extents coincide by accident where an index could be
swapped unnoticed -- Fin = 2, F1 = 3, Fout = 2, k = 4 (w = 3, T = 2 for the upsample images; Fm = 5 for the weight MLP's hidden layer).
The weights hold distinct small integers, so the sums and differences inside the images are exact and every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from spgan import edge_conv, ops

FIN, F1, FOUT, K, W, FM = 2, 3, 2, 4, 3, 5
T = K - W + 1


def _ints(shape, start):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.float32) * 3 + start).reshape(shape).clone()


def _stack(W1):
    """[Wd ; Wc - Wd] of a conv weight [F,2C,1,1] over cat[x_i, x_j - x_i], by hand"""
    F_, C = W1.shape[0], W1.shape[1] // 2
    out = np.zeros((2 * F_, C), np.float32)
    for f in range(F_):
        for c in range(C):
            out[f, c] = W1[f, C + c, 0, 0]
            out[F_ + f, c] = W1[f, c, 0, 0] - W1[f, C + c, 0, 0]
    return out


def _taps(W2):
    """W2i[o, r*F1 + c] == W2[o, c, 0, r]"""
    O, C, _, k = W2.shape
    out = np.zeros((O, k * C), np.float32)
    for o in range(O):
        for c in range(C):
            for r in range(k):
                out[o, r * C + c] = W2[o, c, 0, r]
    return out


def _rank_by_hand(W1, W2):
    Wst, W2i = _stack(W1), _taps(W2)
    return Wst, Wst.T, W2i, W2i.T


def _weight_by_hand(Wh, Wf1, Wf2, Wf3, W2):
    Wst_h, Wst_1, W2i = _stack(Wh), _stack(Wf1), _taps(W2)
    Wm2, Wm3 = Wf2[:, :, 0, 0], Wf3[:, :, 0, 0]
    return Wst_h, Wst_1, np.concatenate([Wst_h, Wst_1]).T, Wm2, Wm2.T, Wm3, Wm3.T, W2i, W2i.T


def _upsample_by_hand(W1, V):
    C, k = W1.shape[1] // 2, V.shape[3] // 2
    w = W1.shape[3]
    t_ = k - w + 1
    F2 = V.shape[0]
    Wc1, Wd1 = np.zeros((4 * C, C), np.float32), np.zeros((4 * C, w * C), np.float32)
    Vc, Vd, V2p = np.zeros((F2, C), np.float32), np.zeros((F2, k * C), np.float32), np.zeros((F2, t_ * 4 * C), np.float32)
    for o in range(4 * C):
        for c in range(C):
            Wc1[o, c] = sum(W1[o, c, 0, t] for t in range(w))
            for t in range(w):
                Wd1[o, t * C + c] = W1[o, C + c, 0, t]
    for f in range(F2):
        for c in range(C):
            Vc[f, c] = sum(V[f, c, 0, j] for j in range(k))
            for j in range(k):
                Vd[f, j * C + c] = V[f, C + c, 0, j]
        # the reference reads the [4C, T] chain per point as (2C, k): flat position o*T + t = c'*k + j feeds conv2's tap k + j of channel c'
        for o in range(4 * C):
            for t in range(t_):
                cp, j = divmod(o * t_ + t, k)
                V2p[f, t * 4 * C + o] = V[f, cp, 0, k + j]
    return Wc1, Wd1, Wd1.T, Vc, Vd, Vd.T, V2p, V2p.T, Wc1.T, Vc.T


BUILDERS = {
    "rank": (lambda ws: edge_conv.rank_images(*ws), _rank_by_hand, [(F1, 2 * FIN, 1, 1), (FOUT, F1, 1, K)]),
    "upsample": (lambda ws: edge_conv.upsample_images(*ws, ws[0].shape[1] // 2, ws[1].shape[3] // 2), _upsample_by_hand,
                 [(4 * FIN, 2 * FIN, 1, W), (2 * FOUT, 2 * FIN, 1, 2 * K)]),
    "weight": (lambda ws: edge_conv.weight_images(*ws), _weight_by_hand,
               [(FIN, 2 * FIN, 1, 1), (F1, 2 * FIN, 1, 1), (FM, F1, 1, 1), (FIN, FM, 1, 1), (FOUT, FIN, 1, K)]),
}


@pytest.fixture(params=list(BUILDERS))
def case(request):
    """One builder on an empty cache; what the cache held before is kept alive and put back, so that this file frees nothing of other tests"""
    held = {name: dict(cache) for name, cache in edge_conv._IMAGES.items()}
    for cache in edge_conv._IMAGES.values():
        cache.clear()
    yield BUILDERS[request.param]
    for name, cache in edge_conv._IMAGES.items():
        cache.clear()
        cache.update(held[name])


def _weights(shapes, start=1):
    return [_ints(s, start + 1000 * i) for i, s in enumerate(shapes)]


def _check(img, by_hand, ws):
    want = by_hand(*[w.numpy() for w in ws])
    assert len(img) == len(want)
    for i, (a, b) in enumerate(zip(img, want)):
        assert tuple(a.shape) == b.shape, i
        assert torch.equal(a, torch.from_numpy(np.ascontiguousarray(b))), i


def _entries():
    return sum(len(cache) for cache in edge_conv._IMAGES.values())             # one builder per test: its dictionary


def _fresh(new, old):
    assert new is not old and all(a is not b for a, b in zip(new, old))


def test_images_by_hand_and_hit(case):
    call, by_hand, shapes = case
    ws = _weights(shapes)
    img = call(ws)
    _check(img, by_hand, ws)
    again = call(ws)
    assert again is img and all(a is b for a, b in zip(again, img))          # unchanged weights: the very same tensors


def test_stale_after_inplace_write(case):
    call, by_hand, shapes = case
    for i in range(len(shapes)):                                             # whichever weight is written
        ws = _weights(shapes)
        old = call(ws)
        epoch = ops.weights_epoch_of(ws[i])
        ws[i].view(-1)[1:3].add_(7.0)                                        # torch's version counter moves, the epoch does not
        assert ops.weights_epoch_of(ws[i]) == epoch
        new = call(ws)
        _fresh(new, old)
        _check(new, by_hand, ws)


def test_stale_after_optimiser_epoch(case):
    call, by_hand, shapes = case
    for i in range(len(shapes)):
        ws = _weights(shapes)
        old = call(ws)
        versions = [w._version for w in ws]
        ws[i].data.copy_(_ints(shapes[i], 5 + 10 * i))                       # as a HIP optimiser step: invisible to torch's version counter
        assert [w._version for w in ws] == versions
        ops.bump_weights_epoch(ws[i])
        new = call(ws)
        _fresh(new, old)
        _check(new, by_hand, ws)


def test_other_shape_at_the_same_address(case):
    call, by_hand, shapes = case
    ws = _weights(shapes)
    old = call(ws)
    last = ws[-1]
    half = (shapes[-1][0] // 2,) + tuple(shapes[-1][1:])
    small = last.view(-1)[:last.numel() // 2].view(half)                     # same data_ptr, same storage and version counter, fewer rows
    assert small.data_ptr() == last.data_ptr() and small._version == last._version
    new = call(ws[:-1] + [small])
    _fresh(new, old)
    _check(new, by_hand, ws[:-1] + [small])


def test_cap(case):
    call, by_hand, shapes = case
    keep, most = [], 0
    for n in range(65):                                                      # 65 weight sets alive at once: 65 distinct keys
        ws = _weights(shapes, start=n)
        keep.append(ws)
        img = call(ws)
        most = max(most, _entries())
        assert _entries() <= 64
    assert most == 64
    _check(img, by_hand, keep[-1])
    assert call(keep[-1]) is img
