"""The entry walk of query_kernel_r counted on the device: rounds, rounds with a second pass over the
entries, second passes in which a lane finds hits.  Needs a measuring build with the counters compiled in, selected at run time:

    make -C cuclark_amd/csrc variant VARIANT_FLAGS="-DMIC_X=264"      # 8: the counters, 256: the walk of the rounds before 11
    MIC_LIB_PATH=cuclark_amd/csrc/obj_var/libmi_clark_var.so python tools/entry_walk_counters.py [--layout super2]

Runs the headline launch of tools/two_part_profile.py (bench.py's table and reads) twice and prints one JSON line more."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import two_part_profile
    from cuclark_amd import _lib
    sys.argv = ["two_part_profile.py", "--set", "n001", "--launches", "2", "--warmup", "0"] + sys.argv[1:]
    two_part_profile.main()
    lib = C.CDLL(_lib.LIB_PATH)
    if not hasattr(lib, "mic_debug_entry_walk"):
        sys.exit("entry_walk_counters.py: the library has no counters (build it with -DMIC_X=8 and select it with MIC_LIB_PATH)")
    out = (C.c_ulonglong * 3)()
    assert lib.mic_debug_entry_walk(out, 0) == 0
    rounds, second, hits = int(out[0]), int(out[1]), int(out[2])
    print(json.dumps({"launches": 2, "rounds": rounds, "rounds_with_a_second_pass": second, "second_passes_with_hits": hits,
                      "share_second_pass": round(second / max(rounds, 1), 5), "share_of_those_with_hits": round(hits / max(second, 1), 5)}), flush=True)


if __name__ == "__main__":
    main()
