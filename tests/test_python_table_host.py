"""The host side of the table contrast's Python surface, without a GPU: the run configuration's optional entries, the
extension's new routine beside the reference's five, and the keywords of seabreezediag.diag reaching it."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, gpu_visible

PW = os.path.join(ROOT, "python_wrapper")


def _built():
    return any(f.startswith("seabreeze.") and f.endswith(".so") for f in os.listdir(PW))


def _import_surface():
    if PW not in sys.path:
        sys.path.insert(0, PW)
    import seabreeze
    import seabreezediag
    assert os.path.dirname(seabreeze.__file__) == PW, seabreeze.__file__
    return seabreeze, seabreezediag


def test_run_configuration_entries(tmp_path):
    """run.conf.example shows both entries commented out; uncommented they read as booleans, absent they are off."""
    import importlib.util
    import types
    text = open(os.path.join(PW, "run.conf.example")).read()
    assert "# table_contrast = true" in text and "# keep_windows = true" in text
    # configdir imports its sibling ncio relatively: load it as part of a stand-in package that does not import the extension
    pkg = types.ModuleType("sb_cfg_pkg")
    pkg.__path__ = [os.path.join(PW, "seabreezediag")]
    sys.modules["sb_cfg_pkg"] = pkg
    try:
        spec = importlib.util.spec_from_file_location("sb_cfg_pkg.configdir", os.path.join(PW, "seabreezediag", "configdir.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["sb_cfg_pkg.configdir"] = mod
        spec.loader.exec_module(mod)
        off = tmp_path / "off.conf"
        off.write_text(text)
        cfg = mod.Config(str(off))
        assert cfg.get("table_contrast", False) is False and cfg.get("keep_windows", False) is False
        on = tmp_path / "on.conf"
        on.write_text(text.replace("# table_contrast = true", "table_contrast = true").replace("# keep_windows = true", "keep_windows = true"))
        cfg = mod.Config(str(on))
        assert cfg.table_contrast is True and cfg.keep_windows is True
    finally:
        for k in [k for k in sys.modules if k.startswith("sb_cfg_pkg")]:
            del sys.modules[k]


@pytest.mark.skipif(not _built(), reason="python_wrapper extension not built")
def test_extension_routine_and_keywords():
    seabreeze, sbd = _import_surface()
    assert seabreeze.set_table_contrast.__doc__.splitlines()[0].strip() == "set_table_contrast(on,[keep_windows])"
    assert seabreeze.last_launches.__doc__.splitlines()[0].strip() == "n = last_launches()"
    if gpu_visible():
        pytest.skip("a GPU is visible here: the rest is tests/test_python_table_gpu.py")
    # without a GPU the keyword reaches the extension, whose sb_create fails: the Python layer raises, before any step
    z = np.zeros((6, 8), np.float32)
    with pytest.raises(RuntimeError, match="set_table_contrast"):
        sbd.diag(1, z, z, z, np.arange(8.0), np.arange(6.0), np.array([700.0]), z[None, None], z[None, None], z[None], None,
                 table_contrast=True)
