"""Stand-in for the `lpips` package at fixture-generation time: metrics/calculate_lpips.py builds
`lpips.LPIPS(net='alex', spatial=True)` at import. The package is not available, so this is the
plain-torch restatement of tests/lpips_torch.py with the seeded weights of tests/lpips_inputs.py."""
from tests import lpips_inputs as _I
from tests import lpips_torch as _T


def LPIPS(net='alex', spatial=False, **kw):
    assert net == 'alex', net
    return _T.Net(_I.make_lpips_sd(), spatial=spatial).eval()
