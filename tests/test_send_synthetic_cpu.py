"""CPU: events.synthetic_round's optional send-batch inputs (loss, chance, payload) leave the six base
arrays and the round end exactly as they are without them."""
import numpy as np

from shadow_amd import events as ev


def test_loss_generation_leaves_the_base_batch_unchanged():
    base, re0 = ev.synthetic_round(20000, 500, 64, seed=3)
    b, re1, loss = ev.synthetic_round(20000, 500, 64, seed=3, loss=0.05)
    assert re0 == re1 and set(b) == set(base) | {"chance", "payload_size"}
    for k, v in base.items():
        assert v.dtype == b[k].dtype and np.array_equal(v, b[k]), k
    assert b["chance"].dtype == np.float64 and b["chance"].min() >= 0.0 and b["chance"].max() < 1.0
    assert b["payload_size"].dtype == np.uint32 and 0.05 < (b["payload_size"] == 0).mean() < 0.15
    assert loss.dtype == np.float32 and loss.shape == (64, 64)
    assert loss.min() >= 0.0 and loss.max() < 0.1 and abs(float(loss.mean()) - 0.05) < 0.005
    # loss 0: a table of zeros (nothing can be dropped), the same draws
    b0, _, loss0 = ev.synthetic_round(20000, 500, 64, seed=3, loss=0.0)
    assert not loss0.any() and np.array_equal(b0["chance"], b["chance"])
