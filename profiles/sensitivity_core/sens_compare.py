"""Compare two dumps of sens_dump.py bit for bit: python profiles/sensitivity_core/sens_compare.py PARENT.npz NEW.npz"""
import re
import sys

import numpy as np

a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
values = finite = differ = texts = 0
bad = []
for key in a.files:
    x, y = a[key], b[key]
    if key.endswith("/raised"):  # (object addresses in a message differ from process to process)
        texts += 1
        if re.sub(rb'0x[0-9a-f]+', b'0x', bytes(x)) != re.sub(rb'0x[0-9a-f]+', b'0x', bytes(y)):
            bad.append((key, bytes(x).decode(), bytes(y).decode()))
        continue
    if x.shape != y.shape or x.dtype != y.dtype:
        bad.append((key, x.shape, y.shape))
        continue
    u, v = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
    values += x.size
    finite += int(np.isfinite(x.astype(np.float64)).sum())
    n = int((u != v).sum())
    differ += n
    if n:
        bad.append((key, n))
cases = len({k.rsplit("/", 1)[0] for k in a.files})
print(f"{cases} cases, {len(a.files) - texts} arrays, {values} values ({finite} finite), {differ} differ; "
      f"{texts} refusal texts, {sum(1 for q in bad if len(q) == 3 and isinstance(q[1], str))} differ")
for q in bad:
    print("  DIFFERS", q)
sys.exit(1 if bad else 0)
