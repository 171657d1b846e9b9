"""Generates tests/golden/ref_kmeans_items.json: the names that tests/test_integration_glue.py checks the Rust adapters against,
listed from the reference's rust/lance-index/src/vector/kmeans.rs -- its function names (and which are `pub`), the variants of
KMeanInit with their payload types, and the fields of KMeansParams with their types.  The test matches its recorded patterns
against these names wherever the reference tree is not available.

Run where the reference tree is present: python tests/golden/make_ref_kmeans_items.py <reference>/rust/lance-index/src/vector/kmeans.rs
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def block(src, head):
    a = src.index(head)
    return src[a:src.index("\n}", a)]


def items(src):
    return {"fns": sorted(set(re.findall(r"\bfn (\w+)\s*[<(]", src))),
            "pub_fns": sorted(set(re.findall(r"\bpub fn (\w+)\s*[<(]", src))),
            "KMeanInit": {m.group(1): m.group(2) for m in re.finditer(r"^\s*(\w+)(?:\((.*)\))?,\s*$", block(src, "pub enum KMeanInit {"), re.M)},
            "KMeansParams": {m.group(1): m.group(2) for m in re.finditer(r"^\s*pub (\w+): (.+),\s*$", block(src, "pub struct KMeansParams {"), re.M)}}


def render(it):
    """The recorded names written back as the declarations they were listed from (what the test's patterns match)."""
    lines = [f"fn {f}(" for f in it["fns"]] + [f"pub fn {f}(" for f in it["pub_fns"]]
    lines += [f"{v}({p})," if p else f"{v}," for v, p in it["KMeanInit"].items()]
    lines += [f"pub {f}: {t}," for f, t in it["KMeansParams"].items()]
    return "\n".join(lines)


if __name__ == "__main__":
    src = open(sys.argv[1]).read()
    json.dump(items(src), open(os.path.join(HERE, "ref_kmeans_items.json"), "w"), indent=1)
