"""The drop-in claim, executed: the reference's OWN callers -- run.py's imports, train.train() with its optimisers /
DataLoader / Logger / DataParallelWithCallback(device_ids=...), reconstruction.generate, transfer.transfer_one +
normalize_kp, Logger.save_cpk / load_cpk -- run unmodified on top of monkey-net_amd/modules and
monkey-net_amd/sync_batchnorm (kernels on the CPU emulator) and reproduce what the reference recorded with its own
modules.  The scenarios need a checkout of the reference (the launcher test only a stand-in of its layout); each scenario is a
fresh process (tests/dropin_worker.py) because the package names collide with the ones this pytest session has already
imported."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MNK_REFERENCE_ROOT", "/root/reference")

# the tests that execute the reference's own scripts; the launcher test below builds its own stand-in of the tree's layout
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "modules")),
                                     reason="needs a checkout of the reference (MNK_REFERENCE_ROOT)")


def _run(scenario, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dropin_worker.py"), scenario], env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("DROPIN_RESULT ")][-1]
    return json.loads(line[len("DROPIN_RESULT "):])


@needs_reference
def test_reference_run_py_imports_resolve_to_the_drop_in():
    assert _run("imports")["ok"]


@needs_reference
def test_reference_train_loop_and_checkpoint_round_trip():
    res = _run("train")
    assert len(res["report"]) == 3


@needs_reference
def test_reference_reconstruction_generate():
    res = _run("reconstruction")
    assert res["max_err"] < 2e-5


@needs_reference
def test_reference_transfer_one_with_normalize_kp():
    res = _run("transfer")
    assert res["video_prediction"] < 5e-5


@needs_reference
def test_batched_transfer_and_device_normalize_kp_match_the_reference_loop():
    res = _run("transfer_batched")
    assert res["video_prediction"] < 2e-5 and res["repair_var"] < 2e-6


def test_launcher_puts_the_drop_in_first(tmp_path):
    """monkey-net_amd/run_reference.py: `python run.py` would resolve `modules` in the script's own directory.  The script
    sits in a stand-in of the reference tree's layout: `modules/` without __init__.py (generator.py, prediction_module.py)
    and the `sync_batchnorm` package; the stand-ins of what the drop-in replaces raise if they are ever imported."""
    script = tmp_path / "probe.py"
    script.write_text("import modules.generator, modules.prediction_module, sync_batchnorm, sys\n"
                      "print(modules.generator.__file__); print(modules.prediction_module.__file__); "
                      "print(sync_batchnorm.__file__); print(sys.argv[1:])\n")
    (tmp_path / "modules").mkdir()
    (tmp_path / "modules" / "generator.py").write_text("raise ImportError('the stand-in, not the drop-in, was imported')\n")
    (tmp_path / "modules" / "prediction_module.py").write_text("PREDICTION_MODULE = True\n")
    (tmp_path / "sync_batchnorm").mkdir()
    (tmp_path / "sync_batchnorm" / "__init__.py").write_text("raise ImportError('the stand-in, not the drop-in, was imported')\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "monkey-net_amd", "run_reference.py"), str(script), "--config",
                          "x.yaml"], capture_output=True, text=True, timeout=300,
                         env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE")})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert "monkey-net_amd/modules/generator.py" in lines[0]
    assert str(tmp_path) in lines[1] and "prediction_module" in lines[1]
    assert "monkey-net_amd/sync_batchnorm" in lines[2]
    assert lines[3] == "['--config', 'x.yaml']"
