#!/usr/bin/env python3
"""Regenerates ref_options.json: the option names that the reference's MATLAB parsers accept (the labels of the first
`switch upper(varargin{i})` block of SALSA/SALSA_v2.m, SALSA/CSALSA_v2.m and SALSA/CoRAL_v2.m), in file order, parsed
with the same helpers tests/test_matlab_shims.py uses.  tests/test_matlab_shims.py checks its option lists against it.

    python tests/golden/make_ref_options.py REFERENCE_CHECKOUT
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_matlab_shims import REF_FILES, _case_labels, _first_switch, matlab_code  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
out = {rel: _case_labels(_first_switch(matlab_code(os.path.join(sys.argv[1], rel)))) for rel in sorted(REF_FILES.values())}
with open(os.path.join(HERE, "ref_options.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
for rel, labels in out.items():
    print(rel, len(labels))
