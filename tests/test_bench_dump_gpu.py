"""bench.py --dump-outputs on a real engine: the dump reads the parameters after the step's
deferred AdamW update and leaves that update pending, so whatever runs after it (the `--full`
legs: the AdamW pass roofline_hbm times returns at once when nothing is pending) sees the
engine as the timed steps left it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_dump_outputs_leaves_the_deferred_update_pending(pkg, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import bench
    L = pkg.lib
    B, SEQ, H = 4, 16, 64
    eng = pkg.engine.VQAEngine(pkg.synthetic.make_state_dict("resnet50", seed=0), vision="resnet50", batch=B,
                               seq_len=SEQ, image_size=H, dropout=0.1, seed=0, pipeline=False, warmup=2, total=10)
    assert eng.defer_opt
    eng.load_batch(pkg.synthetic.make_batch(B, SEQ, H, seed=1))
    eng.train_step()
    eng.train_step()
    torch.cuda.synchronize()
    names = ("P32", "M", "V", "VMAX", "P16", "opt_state")
    before = {k: getattr(eng, k).clone() for k in names}
    assert float(eng.opt_state[L.ST_PENDING]) == 1.0
    bench.dump_outputs(str(tmp_path), eng)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(eng, k), before[k]), k
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["grad_norm", "log_probs", "loss", "params_sample"]
    np.testing.assert_array_equal(got["log_probs"], eng.LOGP.cpu().numpy())
    assert got["loss"][0] == float(eng.LOSS.item()) and got["grad_norm"][0] == np.float32(eng.last_grad_norm())
    # the sample is the parameters with the pending update applied, and differs from the stale ones
    eng.flush_optimizer()
    torch.cuda.synchronize()
    assert float(eng.opt_state[L.ST_PENDING]) == 0.0
    n = eng.P32.numel()
    idx = np.sort(np.random.default_rng(0).integers(0, n, size=min(n, bench.DUMP_PARAMS)))
    np.testing.assert_array_equal(got["params_sample"], eng.P32.cpu().numpy()[idx])
    assert not np.array_equal(got["params_sample"], before["P32"].cpu().numpy()[idx])
