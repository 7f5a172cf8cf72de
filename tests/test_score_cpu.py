"""The host side of device scoring: perplexity.measure_device against a fake model whose score() is
numpy -- the chunking and the ignore_first_n arithmetic give measure()'s positions, count and loss."""
import math

import numpy as np
import pytest

from rwkv_lib import REPO  # noqa: F401  (puts the package on sys.path)
from rwkv_cpp import perplexity

V = 50


class FakeModel:
    """A 'model' whose logits after a token sequence are a fixed function of a running hash of it;
    eval() carries the hash as the state, score() continues the device-resident one."""

    def __init__(self):
        self.dev = 0
        self.calls = []

    @staticmethod
    def _step(h, token):
        return (h * 31 + token + 7) % 10007

    @staticmethod
    def _logits(h):
        return (np.random.default_rng(h).standard_normal(V) * 3).astype(np.float32)

    def eval(self, token, state_in, state_out=None, logits_out=None, use_numpy=True):
        h = self._step(0 if state_in is None else int(state_in[0]), token)
        return self._logits(h), np.array([h], np.float32)

    def reset_state(self):
        self.dev = 0

    def score(self, tokens, targets=None, want_logits=False):
        assert targets is not None and len(targets) == len(tokens) and len(tokens) > 0
        self.calls.append(len(tokens))
        rows = []
        for t in tokens:
            self.dev = self._step(self.dev, t)
            rows.append(self._logits(self.dev))
        losses = np.array([perplexity.cross_entropy(r, t) for r, t in zip(rows, targets)], np.float64)
        return losses, np.array([np.argmax(r) for r in rows], np.uint32), None


TOKENS = [int(t) for t in np.random.default_rng(3).integers(0, V, 41)]


@pytest.mark.parametrize('chunk', [1, 7, 40, 1024])
@pytest.mark.parametrize('ignore_first_n', [0, 1, 2, 8, 20, 39])
def test_measure_device_scores_the_positions_of_measure(chunk, ignore_first_n):
    loss, ppl, n = perplexity.measure(FakeModel(), TOKENS, ignore_first_n)
    m = FakeModel()
    m.dev = 1234  # a stale device state: measure_device starts from a fresh one
    dloss, dppl, dn = perplexity.measure_device(m, TOKENS, ignore_first_n, chunk=chunk)
    assert dn == n
    assert abs(dloss - loss) <= 1e-12 and dppl == math.exp(dloss)
    # tokens[:-1] in chunks, in order
    T = len(TOKENS) - 1
    assert m.calls == [min(chunk, T - i) for i in range(0, T, chunk)]


def test_measure_device_refuses_what_measure_refuses():
    for fn in (perplexity.measure, perplexity.measure_device):
        with pytest.raises(ValueError):
            fn(FakeModel(), TOKENS[:9], 8)
        with pytest.raises(ValueError):
            fn(FakeModel(), TOKENS[:1], 0)
    with pytest.raises(ValueError):
        perplexity.measure_device(FakeModel(), TOKENS, 0, chunk=0)


def test_cli_has_the_device_flag(monkeypatch):
    seen = {}

    def fake(name):
        def f(model, tokens, ignore_first_n=0, **kw):
            seen['which'] = name
            return 1.0, math.e, len(tokens) - 1
        return f

    import rwkv_cpp
    from rwkv_cpp import world_tokenizer
    monkeypatch.setattr(perplexity, 'measure', fake('measure'))
    monkeypatch.setattr(perplexity, 'measure_device', fake('measure_device'))
    monkeypatch.setattr(rwkv_cpp, 'RWKVModel', lambda lib, path: object())
    monkeypatch.setattr(rwkv_cpp, 'load_rwkv_shared_library', lambda: None)
    monkeypatch.setattr(world_tokenizer, 'get_world_tokenizer', lambda vocab: (None, lambda text: [1, 2, 3, 4]))
    perplexity.main(['model.bin', __file__, '0'])
    assert seen['which'] == 'measure'
    perplexity.main(['model.bin', __file__, '0', '--device'])
    assert seen['which'] == 'measure_device'
