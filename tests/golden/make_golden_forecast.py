#!/usr/bin/env python3
"""
Writes tests/golden/forecast_display.json -- runs ONLY in the build container (needs the reference).

The values with which the reference's forecast GIFs are drawn, read from the reference's own file ``py4cast/utils.py`` WITHOUT running
it (it imports gif, cartopy and the datasets): the module is parsed, the literal ``PARAMS_INFO`` table gives colormap, vmin and vmax
per parameter, and the three constants of ``plot_frame`` / ``make_gif`` are read from the expressions that hold them:

    cmap = "plasma"                                  the colormap of a parameter the table lacks (auto-scaled: vmin, vmax = None, None)
    if param == "tp": np.where(data < 0.5, ...)      the precipitation floor
    if feature == "aro_t2m_2m": pred - 273.15        the offset of the feature shown in degrees Celsius

The file holds values only: parameter -> colormap name, vmin, vmax, floor; the default row; feature name -> offset.

    python tests/golden/make_golden_forecast.py
"""
import ast
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PY4CAST_REFERENCE", "/root/reference")


def function(tree, name):
    (fn,) = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    return fn


def guarded(fn, variable):
    """(the string a variable is compared with, the body of that ``if``) for ``if <variable> == "<string>":`` in a function"""
    for node in ast.walk(fn):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.left, ast.Name) \
                and node.test.left.id == variable and isinstance(node.test.ops[0], ast.Eq):
            return node.test.comparators[0].value, node.body
    raise SystemExit(f"no `if {variable} == ...` in {fn.name}")


def main():
    with open(os.path.join(REF, "py4cast", "utils.py")) as f:
        tree = ast.parse(f.read())
    (table,) = [n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "PARAMS_INFO"]
    table = ast.literal_eval(table)
    frame, gif = function(tree, "plot_frame"), function(tree, "make_gif")

    floor_param, body = guarded(frame, "param")
    (floor,) = [n.comparators[0].value for b in body for n in ast.walk(b) if isinstance(n, ast.Compare) and isinstance(n.ops[0], ast.Lt)]
    (default,) = {n.value.value for n in ast.walk(frame) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "cmap"
                  and isinstance(n.value, ast.Constant)}
    offset_feature, body = guarded(gif, "feature")
    (offset,) = {n.right.value for b in body for n in ast.walk(b) if isinstance(n, ast.BinOp) and isinstance(n.op, ast.Sub)
                 and isinstance(n.right, ast.Constant)}

    params = {p: {"cmap": row["cmap"], "vmin": float(row["vmin"]), "vmax": float(row["vmax"]), "floor": float(floor) if p == floor_param else None}
              for p, row in table.items()}
    assert floor_param in params
    out = {"params": params, "default": {"cmap": default, "vmin": None, "vmax": None, "floor": None},
           "offsets": {offset_feature: -float(offset)}}
    path = os.path.join(HERE, "forecast_display.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(params)} parameters, floor {floor} for {floor_param}, offset {-float(offset)} for {offset_feature}")


if __name__ == "__main__":
    main()
