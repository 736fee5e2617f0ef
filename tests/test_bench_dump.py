"""bench.py --dump-outputs: one float32 .npy per tenant output, a large output
as the same seeded sample on every call, tenants without an output tensor
skipped."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _corun():
    g = torch.Generator().manual_seed(7)
    big = torch.randn(3 * (1 << 19) + 5, generator=g).to(torch.bfloat16)  # > DUMP_SAMPLE elements

    def runner(out, alt=None):
        """What dump_outputs reads of a runtime/gpu.py Runner: the ABI record
        (c / alt_c device pointers) and the tensors the runner keeps alive."""
        ins = [torch.ones(3), torch.ones(5)]
        cfg = types.SimpleNamespace(c=out.data_ptr() if out is not None else None,
                                    alt_c=alt.data_ptr() if alt is not None else None)
        bufs = ins + [t for t in (out, alt) if t is not None]
        return types.SimpleNamespace(cfg=cfg, buffers=bufs, output=out, alt_output=alt)

    runners = {
        "gemm": runner(torch.randn(8, 12, generator=g).to(torch.bfloat16)),
        "hbm": runner(big),
        "phase": runner(torch.randn(6, generator=g), torch.randn(4, generator=g)),
        "ipc": runner(None),  # the IPC all-reduce runner: its buffers live in the collective
        "coll": types.SimpleNamespace(buf=torch.zeros(4)),  # a torch collective tenant: no runner record
    }
    return types.SimpleNamespace(runners=runners)


def test_dump_outputs_files_and_sample(tmp_path):
    import bench
    c = _corun()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(c, a)
    bench.dump_outputs(c, b)
    assert sorted(os.listdir(a)) == ["gemm.npy", "hbm.npy", "phase.npy", "phase_alt.npy"]
    total = 0
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and x.ndim == 1
        assert np.array_equal(x, y), f  # the same sample every time
        total += x.nbytes
    assert total <= 64 << 20
    gemm = np.load(os.path.join(a, "gemm.npy"))
    assert np.array_equal(gemm, c.runners["gemm"].output.float().reshape(-1).numpy())
    assert np.array_equal(np.load(os.path.join(a, "phase_alt.npy")), c.runners["phase"].alt_output.numpy())
    # the large output: DUMP_SAMPLE elements at sorted seeded indexes
    hbm = np.load(os.path.join(a, "hbm.npy"))
    assert hbm.shape == (bench.DUMP_SAMPLE,)
    idx = torch.randint(c.runners["hbm"].output.numel(), (bench.DUMP_SAMPLE,),
                        generator=torch.Generator().manual_seed(bench.DUMP_SEED), dtype=torch.int64).sort().values
    assert np.array_equal(hbm, c.runners["hbm"].output.float()[idx].numpy())


def test_bench_cli_has_the_contract_options():
    """--full, --dump-outputs and --budget-s parse (argparse runs before
    anything touches the GPU), and a plain run is the default."""
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, p.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs DIR", "--budget-s"):
        assert opt in p.stdout, opt
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_headline_outputs_fit_the_dump_budget():
    """The 4mix outputs (three sampled tensors and the GEMV's 8192 floats)
    stay far below 64 MB."""
    import bench
    from pbs_amd.bench.corun import MIXES
    assert len(MIXES["4mix"]["tenants"]) * bench.DUMP_SAMPLE * 4 <= 64 << 20
