"""
Records tests/golden/noisy_return_codes.json: the return code of every case of tests/test_noisy_return_codes.py from the
library that QHEA_LIB names (default: the built one).  Host only, nothing is launched.
    python tests/golden/make_noisy_return_codes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                   # noqa: E402
from tests import test_noisy_return_codes as T                  # noqa: E402

if __name__ == '__main__':
    table = T.all_codes(_lib.load())
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with open(out, 'w') as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f"{sum(len(v) for v in table.values())} cases from {_lib.LIB_PATH} -> {out}")
