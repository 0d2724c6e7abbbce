"""bench.py --dump-outputs: the byte budget and the seeded sample."""
import numpy as np
import torch


def test_dump_outputs_budget_and_seeded_sample(tmp_path, monkeypatch):
    """The first array is written whole while it fits, the others share what is left as sorted samples of
    their flattened elements; a second call picks the same elements; nothing exceeds the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 1000)
    g = torch.Generator().manual_seed(3)
    arrays = {"x": torch.rand((2, 3, 10, 10), generator=g),            # 600 elements: whole
              "a": torch.rand((3, 10, 10), generator=g),               # 300 elements, 200 allowed
              "b": torch.rand((3, 10, 10), generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "d1"), arrays)
    bench.dump_outputs(str(tmp_path / "d2"), arrays, suffix="_rank1")
    out = {n: np.load(tmp_path / "d1" / f"{n}.npy") for n in arrays}
    assert all(v.dtype == np.float32 for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 4 * 1000
    np.testing.assert_array_equal(out["x"], arrays["x"].numpy())
    assert out["a"].shape == (200,) and out["b"].shape == (200,)
    flat = arrays["a"].numpy().reshape(-1)
    np.testing.assert_array_equal(flat[np.isin(flat, out["a"])], out["a"])      # elements of a, in a's order
    for n in arrays:
        np.testing.assert_array_equal(out[n], np.load(tmp_path / "d2" / f"{n}_rank1.npy"))
