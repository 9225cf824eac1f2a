import os
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')


@pytest.fixture(scope='session')
def pkg():
    # torch before the library: torch links its own HIP runtime by the unversioned name libamdhip64.so, so a library loaded first would
    # bring the system runtime in beside it, and in a run of the whole suite the GPU tests' library would then find no device
    import torch  # noqa: F401
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope='session')
def engine(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    eng = pkg.Engine(0)
    yield eng
    eng.close()
