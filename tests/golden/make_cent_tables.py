"""Regenerates tests/golden/cent_reference_tables.npz.  Run ONLY in the build container:

    python -B tests/golden/make_cent_tables.py

Source (data only; no reference source text is stored): the default parameter tables - the layers' initial weights - of
the reference's ``CENTCharge`` (``_default_radii`` in Bohr, ``_default_hardness``, kgcnn/layers/conv/hdnnp_conv.py:85-106)
and ``ElectrostaticEnergyGaussCharge`` (``_default_radii`` in Angstrom, :318-327).  The reference module needs TensorFlow
to import, so the numeric literals and their unit factors are read from its syntax tree and evaluated as NumPy does
(``factor * np.array(values)`` in float64).
"""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _tables():
    tree = ast.parse(open(os.path.join(REF, "kgcnn", "layers", "conv", "hdnnp_conv.py")).read())
    out = {}
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
        for stmt in cls.body:
            if not (isinstance(stmt, ast.Assign) and isinstance(stmt.targets[0], ast.Name)):
                continue
            name = stmt.targets[0].id
            if name not in ("_default_radii", "_default_hardness"):
                continue
            # factor * np.array([...]) with factor a literal or a literal quotient
            factor = ast.literal_eval(stmt.value.left) if isinstance(stmt.value.left, ast.Constant) else \
                ast.literal_eval(stmt.value.left.left) / ast.literal_eval(stmt.value.left.right)
            values = np.array(ast.literal_eval(stmt.value.right.args[0]))
            out["%s.%s" % (cls.name, name)] = factor * values
    return out


if __name__ == "__main__":
    t = _tables()
    np.savez(os.path.join(HERE, "cent_reference_tables.npz"),
             cent_sigma_bohr=t["CENTCharge._default_radii"], cent_hardness=t["CENTCharge._default_hardness"],
             gauss_sigma_angstrom=t["ElectrostaticEnergyGaussCharge._default_radii"])
    print("fixture written to", HERE)
