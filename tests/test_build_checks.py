"""CPU: checks on the compiled product that need no GPU.

tools/spill_exec_scan.py looks through the device assembly of every kernel file for VGPR spill code that the register allocator put at the head of a join block IN FRONT OF the
`s_or_b64 exec, exec, ...` that re-activates the lanes (round 6: k_lb_pass<2, OpBlockHeads, 8> under a 128-register bound stored its wave-scan values for lane 63 only and every other
lane read a stale scratch slot -- wrong block lists and memory faults).  The product build must not contain the pattern."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "tools", "spill_exec_scan.py")

BAD = """
_Z6kernelv:
; %bb.0:
	s_and_saveexec_b64 s[0:1], s[2:3]
	s_cbranch_execz .LBB0_2
; %bb.1:
	ds_write_b32 v1, v0
.LBB0_2:
	v_writelane_b32 v127, s16, 23
	scratch_store_dword off, v10, off offset:164 ; 4-byte Folded Spill
	s_or_b64 exec, exec, s[0:1]
	s_barrier
	scratch_load_dword v60, off, off offset:164 ; 4-byte Folded Reload
	s_endpgm
"""
GOOD = BAD.replace("\tscratch_store_dword off, v10, off offset:164 ; 4-byte Folded Spill\n\ts_or_b64 exec, exec, s[0:1]\n",
                   "\ts_or_b64 exec, exec, s[0:1]\n\tscratch_store_dword off, v10, off offset:164 ; 4-byte Folded Spill\n")


def test_scanner_sees_a_spill_in_front_of_the_exec_restore(tmp_path):
    bad = tmp_path / "bad.s"; bad.write_text(BAD)
    good = tmp_path / "good.s"; good.write_text(GOOD)
    r = subprocess.run([sys.executable, SCAN, str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "1 spill instruction(s) in front of the exec restore" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, SCAN, str(good)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout


def test_buffer_lists_name_every_devbuf_member_once():
    """gsa_destroy frees what GSA_DEVBUFS (hipFree) and GSA_PINBUFS (hipHostFree) name: every DevBuf member of gsa_ctx and of its two QuerySlots must stand in
    exactly one of the two lists, once, array members element by element, and the lists name nothing else (a member left out leaks with every context)."""
    import re
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "gsalign_amd", "csrc", "gsa_ctx.h")).read())

    def members(struct):
        body = re.search(r"\bstruct %s \{(.*?)\n\};" % struct, src, re.S).group(1)
        out = []
        for stmt in body.split(";"):
            m = re.match(r"\s*DevBuf\s+(.+)$", stmt, re.S)
            for decl in (m.group(1).split(",") if m else []):
                name, dim = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", decl).groups()
                out += [f"{name}[{k}]" for k in range(int(dim))] if dim else [name]
        return out

    declared = members("gsa_ctx") + [f"qs[{i}].{m}" for i in range(2) for m in members("QuerySlot")]
    listed = []
    for macro in ("GSA_DEVBUFS", "GSA_PINBUFS"):
        text = re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)" % macro, src).group(1)
        listed += re.findall(r"X\(([^)]+)\)", text)
    assert len(declared) > 150 and len(set(declared)) == len(declared)
    assert sorted(listed) == sorted(declared), (sorted(set(declared) - set(listed)), sorted(set(listed) - set(declared)), [n for n in set(listed) if listed.count(n) > 1])


def test_product_kernels_have_no_spill_in_front_of_an_exec_restore():
    r = subprocess.run(["make", "-j8", "check-spills"], cwd=os.path.join(ROOT, "gsalign_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), (r.stdout[-3000:], r.stderr[-2000:])
