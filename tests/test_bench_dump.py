"""bench.py --dump-outputs: the files dump_outputs writes, checked on host tensors (no GPU)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_small_and_sampled(tmp_path):
    B = _bench()
    g = torch.Generator().manual_seed(7)
    small = torch.randint(0, 256, (3 * B.DUMP_BLOCK + 17,), generator=g, dtype=torch.uint8)
    big = torch.randint(0, 256, (B.DUMP_HEAD + B.DUMP_SAMPLE + B.DUMP_BLOCK + 5,), generator=g, dtype=torch.uint8)
    sizes = {"compressed_bits": 123, "decompressed_bytes": big.numel()}
    for d in ("a", "b"):
        B.dump_outputs(str(tmp_path / d), "", {"compressed": small, "decompressed": big}, sizes)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a") if f.endswith(".npy")}
    assert sorted(a) == ["compressed.npy", "compressed_block_sums.npy", "decompressed.npy",
                         "decompressed_block_sums.npy", "sizes.npy"]
    for f, x in a.items():                      # the same outputs give the same files
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, np.load(tmp_path / "b" / f)), f
    # an output within the budget is written whole; a larger one as its head + a fixed sample
    assert np.array_equal(a["compressed.npy"], small.numpy().astype(np.float32))
    s = a["decompressed.npy"]
    assert s.shape == (B.DUMP_HEAD + B.DUMP_SAMPLE,)
    assert np.array_equal(s[:B.DUMP_HEAD], big[:B.DUMP_HEAD].numpy().astype(np.float32))
    # every byte enters exactly one block sum (the last block is the remainder)
    for name, x in (("compressed", small), ("decompressed", big)):
        bs = a[f"{name}_block_sums.npy"]
        xn = x.numpy().astype(np.int64)
        assert bs.shape == (-(-x.numel() // B.DUMP_BLOCK),)
        assert bs.sum() == xn.sum()
        assert bs[0] == xn[:B.DUMP_BLOCK].sum() and bs[-1] == xn[x.numel() - x.numel() % B.DUMP_BLOCK:].sum()
    assert a["sizes.npy"].tolist() == [123.0, float(big.numel())]
    assert (tmp_path / "a" / "sizes_names.txt").read_text().split() == list(sizes)
    # one flipped byte anywhere shows in the block sums
    big2 = big.clone()
    big2[-3] ^= 1
    B.dump_outputs(str(tmp_path / "c"), "", {"decompressed": big2}, sizes)
    assert not np.array_equal(np.load(tmp_path / "c" / "decompressed_block_sums.npy"),
                              a["decompressed_block_sums.npy"])
    # the default workload's dump (two outputs of at most 4 GiB each) stays under 64 MB
    worst = 2 * ((B.DUMP_HEAD + B.DUMP_SAMPLE) * 4 + (4 << 30) // B.DUMP_BLOCK * 8)
    assert worst < 64 * 10**6
