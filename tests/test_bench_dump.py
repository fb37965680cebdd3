"""bench.py --dump-outputs: the written arrays (CPU tensors stand in for the device buffers)."""
import os

import numpy as np
import torch

import bench


def _words(bits):
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def test_small_planes_written_whole(tmp_path):
    g = torch.Generator().manual_seed(7)
    d_in = torch.randint(-2**63, 2**63 - 1, (1000,), dtype=torch.int64, generator=g)
    d_eg = torch.randint(-2**63, 2**63 - 1, (3, 5), dtype=torch.int64, generator=g)
    d_st = torch.randint(0, 4, (37, 8), dtype=torch.uint8, generator=g)
    bench.dump_outputs(str(tmp_path), d_in, d_eg, d_st)
    assert sorted(os.listdir(tmp_path)) == ["egress_bits.npy", "ingress_bits.npy", "status.npy"]
    for name, t in (("ingress_bits", d_in), ("egress_bits", d_eg)):
        bits = np.load(tmp_path / f"{name}.npy")
        assert bits.dtype == np.float32 and bits.shape == (t.numel(), 64)
        assert np.array_equal(_words(bits), t.reshape(-1).numpy().view(np.uint64))
    st = np.load(tmp_path / "status.npy")
    assert st.dtype == np.float32 and np.array_equal(st, d_st.reshape(-1).numpy())


def test_large_planes_sampled_the_same_every_time(tmp_path):
    n = 4 * bench.DUMP_WORDS + 13
    d_in = torch.arange(n, dtype=torch.int64) * 6364136223846793005  # (odd multiplier, wraps: distinct words)
    d_eg = d_in.flip(0)
    d_st = (torch.arange(bench.DUMP_STATUS + 5) % 4).to(torch.uint8)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), d_in, d_eg, d_st)
    bench.dump_outputs(str(b), d_in.clone(), d_eg.clone(), d_st.clone(), "_rank0")
    total = 0
    for f in ("ingress_bits", "egress_bits", "status"):
        x, y = np.load(a / f"{f}.npy"), np.load(b / f"{f}_rank0.npy")
        assert np.array_equal(x, y)
        total += os.path.getsize(a / f"{f}.npy")
    assert total <= 64 * 10**6
    bits = np.load(a / "ingress_bits.npy")
    assert bits.shape == (bench.DUMP_WORDS, 64)
    # the sample is a subset of the plane's words, in buffer order
    all_words = d_in.numpy().view(np.uint64)
    pos = {int(w): i for i, w in enumerate(all_words)}
    idx = [pos[int(w)] for w in _words(bits)]
    assert idx == sorted(idx) and len(set(idx)) == len(idx)
