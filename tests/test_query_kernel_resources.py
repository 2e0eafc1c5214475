"""The registers, scratch and LDS of the sixteen instantiations of the per-run query kernel (cuclark_amd/csrc/mic_kernels.hip:
query_kernel_r<k, m, one-strand?, part?>), read from the kernel descriptors of the device assembly that `make asm` cross-compiles for
gfx950 with the product's own flags - one compile per session, no GPU.  The kernel runs 8 wavefronts per SIMD: that holds up to 64
vector registers, with nothing spilled to scratch memory, and with four wavefronts' staging areas in a block's LDS.  The scalar
registers are at the file's end already: no instantiation may take more than it did at the commit before this test
(tests/golden/query_kernel_resources.json, written by this file run as a script on that commit).  Resource numbers only: nothing here
looks at instructions."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_kernel_resources.json")
INSTANCES = [(k, m, fwd, part) for k, m in ((31, 20), (27, 20), (32, 20), (0, 0)) for fwd in (False, True) for part in (False, True)]
FIELDS = {"vgpr": "vgpr_count", "sgpr": "sgpr_count", "private": "private_segment_fixed_size", "lds": "group_segment_fixed_size",
          "vgpr_spill": "vgpr_spill_count", "sgpr_spill": "sgpr_spill_count"}


def instance_name(k, m, fwd, part):
    return "query_kernel_r<%d, %d, %s, %s>" % (k, m, "true" if fwd else "false", "true" if part else "false")


def _mangled(k, m, fwd, part):
    """the instantiation's part of the symbol (the namespace in front of it is the compiler's business)"""
    return "14query_kernel_rILi%dELi%dELb%dELb%dEE" % (k, m, fwd, part)


def kernel_resources(asm_text):
    """name -> resources, from the kernels' entries in the code object's metadata (one `- .agpr_count: ...` block per kernel)"""
    out = {}
    for block in re.split(r"\n  - (?=\.agpr_count:)", asm_text):
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M)
        if not name:
            continue
        vals = {}
        for key, field in FIELDS.items():
            v = re.search(r"^\s*\.%s:\s*(\d+)" % field, block, re.M)
            assert v, (name.group(1), field)
            vals[key] = int(v.group(1))
        out[name.group(1)] = vals
    return out


def compile_resources(workdir):
    asm = os.path.join(str(workdir), "mic_kernels.s")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "cuclark_amd", "csrc"), "asm", "ASM_OUT=" + asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    by_symbol = kernel_resources(open(asm).read())
    out = {}
    for i in INSTANCES:
        found = [v for sym, v in by_symbol.items() if _mangled(*i) in sym]
        assert len(found) == 1, (instance_name(*i), len(found))
        out[instance_name(*i)] = found[0]
    return out


@pytest.fixture(scope="session")
def resources(tmp_path_factory):
    return compile_resources(tmp_path_factory.mktemp("query_kernel_asm"))


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: instance_name(*i))
def test_instantiation_keeps_its_occupancy_and_its_scalar_registers(inst, resources):
    name = instance_name(*inst)
    got, parent = resources[name], json.load(open(GOLDEN))["kernels"][name]
    print(name, got, "parent", parent)
    assert got["vgpr"] <= 64, (name, got)                      # 8 wavefronts per SIMD
    assert got["private"] == 0 and got["vgpr_spill"] == 0, (name, got)          # nothing in scratch memory
    assert got["lds"] <= 19904, (name, got)                    # 8 blocks of 4 wavefronts per CU
    assert got["sgpr"] <= parent["sgpr"], (name, got, parent)


if __name__ == "__main__":     # python tests/test_query_kernel_resources.py WORKDIR: write the golden file from this tree
    res = compile_resources(sys.argv[1])
    with open(GOLDEN, "w") as f:
        json.dump({"arch": "gfx950", "source": "cuclark_amd/csrc/mic_kernels.hip", "kernels": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, v in res.items():
        print(name, v)
