"""tests/golden/rearrange_materials.json: the reference's five object materials (robogym/envs/rearrange/materials/*.jsonnet with base.libsonnet merged in) as
numbers -- per material the density, friction, solref and solimp of its `geom` entry (null: the entry has none, the compiled world's value is kept), condim and
margin, and the damping and armature of its `joint` entry (a material without one: MuJoCo's defaults, 0 and 0).  robogym_amd/envs/rearrange/materials.py holds the
same table as plain Python values; tests/test_rearrange_materials.py compares the two.  Settings only.  Needs /root/reference; the fixture travels.

Reads the files with `_jsonnet` where that module is importable, otherwise with the minimal reader below for what these files use: one `(import "file") +`
in front of an object, `key: value` and `key+: {...}` members, strings, numbers, `#` comments.

    python tools/gen_golden_rearrange_materials.py
"""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
MATERIALS_DIR = "/root/reference/robogym/envs/rearrange/materials"


def _tokens(text):
    text = re.sub(r"#[^\n]*|//[^\n]*", " ", text)
    return re.findall(r'"[^"]*"|[A-Za-z_]\w*|-?\d+\.?\d*(?:[eE][-+]?\d+)?|\+:|[{}():,+]', text)


def _parse_object(tok, i):
    """tok[i] == "{" -> ({key: (value, merges)}, index after the closing brace)"""
    assert tok[i] == "{", tok[i]
    i += 1
    out = {}
    while tok[i] != "}":
        key = tok[i].strip('"')
        merges = tok[i + 1] == "+:"
        assert tok[i + 1] in (":", "+:"), tok[i + 1]
        i += 2
        if tok[i] == "{":
            value, i = _parse_object(tok, i)
        elif tok[i].startswith('"'):
            value, i = tok[i][1:-1], i + 1
        else:
            value, i = float(tok[i]), i + 1
        out[key] = (value, merges)
        if tok[i] == ",":
            i += 1
    return out, i + 1


def _merge(base, over):
    """jsonnet's `base + over` for objects: a member replaces the base's, `key+:` merges into it"""
    out = dict(base)
    for key, (value, merges) in over.items():
        if merges and key in out and isinstance(value, dict):
            out[key] = (_merge(out[key][0], value), False)
        else:
            out[key] = (value, False)
    return out


def _plain(obj):
    return {k: (_plain(v) if isinstance(v, dict) else v) for k, (v, _) in obj.items()}


def read_material(path):
    try:
        import _jsonnet

        return json.loads(_jsonnet.evaluate_file(path))
    except ImportError:
        pass
    tok = _tokens(open(path).read())
    base, i = {}, 0
    if tok[0] == "(":
        assert tok[1] == "import" and tok[3] == ")" and tok[4] == "+", tok[:5]
        base = read_material(os.path.join(os.path.dirname(path), tok[2].strip('"')))
        base = {k: ({kk: (vv, False) for kk, vv in v.items()} if isinstance(v, dict) else v, False) for k, v in base.items()}
        i = 5
    obj, end = _parse_object(tok, i)
    assert end == len(tok), tok[end:]
    return _plain(_merge(base, obj))


def numbers(value):
    return None if value is None else [float(v) for v in str(value).split()]


def describe(args):
    geom, joint = args.get("geom", {}), args.get("joint", {})
    assert set(args) <= {"geom", "joint"} and set(geom) <= {"condim", "margin", "density", "friction", "solref", "solimp"} and set(joint) <= {"damping", "armature"}, args
    one = lambda v: None if v is None else numbers(v)[0]
    return dict(density=one(geom.get("density")), friction=numbers(geom.get("friction")), solref=numbers(geom.get("solref")), solimp=numbers(geom.get("solimp")),
                condim=int(one(geom["condim"])), margin=one(geom["margin"]), joint_damping=one(joint.get("damping", 0.0)), joint_armature=one(joint.get("armature", 0.0)))


def main():
    names = sorted(f[:-len(".jsonnet")] for f in os.listdir(MATERIALS_DIR) if f.endswith(".jsonnet"))
    out = {n: describe(read_material(os.path.join(MATERIALS_DIR, n + ".jsonnet"))) for n in names}
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_materials.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
