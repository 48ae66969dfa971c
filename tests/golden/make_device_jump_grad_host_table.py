"""
Records tests/golden/device_jump_grad_host_table.json: the return code of every case and the size of every grid point of
tests/test_device_jump_grad_host_table.py from the library that QHEA_LIB names (default: the built one).  Host only, nothing
is launched.
    python tests/golden/make_device_jump_grad_host_table.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from quanonet_amd import _lib                                   # noqa: E402
from tests import test_device_jump_grad_host_table as T         # noqa: E402

if __name__ == '__main__':
    table = T.all_tables(_lib.load())
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with open(out, 'w') as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f"{sum(len(v) for part in table.values() for v in part.values())} entries from {_lib.LIB_PATH} -> {out}")
