"""CPU: tools/scratch_map.py on a hand-written assembly of the shape the compiler emits for rppk2t::rrt_star_kernel_v2 --
spill slots with their reloads and consumers, the two consumer classes DESIGN 6.0h gates on, and the regions between
streaming loops (the loop finder of tools/loop_spill_check.sh)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "scratch_map.py")


def _loop(prologue, rounds):
    out = ["\tglobal_load_dwordx4 v[0:3], v[40:41], off nt"] * prologue
    for _ in range(rounds):
        out += ["\tv_add_u32_e32 v9, v9, v9"] * 70 + ["\tglobal_load_dwordx4 v[0:3], v[40:41], off nt"]
    return out


ASM = "\n".join(
    ["\t.text", "_ZN5other6kernelEv:", "\tscratch_load_dword v1, off, off offset:4 ; 4-byte Folded Reload", "\ts_endpgm",
     "_ZN6rppk2t18rrt_star_kernel_v2EN4rppk3CtxEi:",
     "\tscratch_store_dword off, v5, off offset:128 ; 4-byte Folded Spill",
     "\tscratch_store_dword off, v6, off offset:156 ; 4-byte Folded Spill",
     "\tscratch_store_dwordx2 off, v[10:11], off ; 8-byte Folded Spill"]
    + _loop(2, 3)
    + ["\tscratch_load_dword v7, off, off offset:128 ; 4-byte Folded Reload",
       "\tv_pk_sub_i16 v8, v20, v7 clamp",
       "\tv_mov_b32_e32 v7, 0",
       "\tv_cmp_eq_u32_e32 vcc, v7, v8",                     # v7 was written again: no consumer of the reload
       "\tscratch_load_dword v12, off, off offset:156 ; 4-byte Folded Reload",
       "\tds_bpermute_b32 v13, v12, v14",                    # the reload is the address
       "\tscratch_load_dword v12, off, off offset:156 ; 4-byte Folded Reload",
       "\tds_bpermute_b32 v13, v14, v12",                    # ... the data
       "\tscratch_load_dwordx2 v[16:17], off, off ; 8-byte Folded Reload",
       "\tv_mul_f64 v[18:19], v[16:17], v[16:17]"]
    + _loop(2, 2)
    + ["\tscratch_load_dword v7, off, off offset:128 ; 4-byte Folded Reload",
       "\tglobal_store_dword v[40:41], v7, off",
       "\ts_endpgm", ""])


def test_scratch_map_on_a_synthetic_kernel(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    out = subprocess.run([sys.executable, TOOL, str(p)], check=True, capture_output=True, text=True).stdout
    lines = out.split("\n")
    assert "3 slots, 3 static spills, 5 static reloads, 8 scratch instructions" in lines[0]   # the other kernel is not counted
    assert lines[1].endswith("address: 1")
    assert lines[2].endswith("(qdist): 1")
    rows = {int(l.split()[0]): l.split() for l in lines[4:7]}
    assert rows[128][1:3] == ["1", "2"] and "v_pk_sub_i16:1" in rows[128] and "global_store_dword:1" in rows[128]
    assert not any(t.startswith("v_cmp_eq") for t in rows[128])
    assert rows[156][1:3] == ["1", "2"] and "ds_bpermute_b32:addr:1" in rows[156] and "ds_bpermute_b32:data:1" in rows[156]
    assert rows[0][1:3] == ["1", "1"] and "v_mul_f64:1" in rows[0]
    assert any(l.startswith("2 streaming loops") for l in lines)
    reg = {l[:26].strip(): l.split()[-2:] for l in lines if l.startswith(("before", "between", "loop ", "after"))}
    assert reg["before loop 1"] == ["3", "0"]
    assert reg["loop 1"] == ["0", "0"] and reg["loop 2"] == ["0", "0"]
    assert reg["between loops 1 and 2"] == ["4", "4"]
    assert reg["after loop 2"] == ["1", "1"]


def test_scratch_map_per_file_table(tmp_path):
    g = "\n".join(['\t.file\t1 "/src" "a.inc"', '\t.file\t2 "/src/b.h"',
                   "_ZN6rppk2t18rrt_star_kernel_v2EN4rppk3CtxEi:",
                   "\t.loc\t1 10 3",
                   "\tscratch_store_dword off, v5, off offset:8 ; 4-byte Folded Spill",
                   "\t.loc\t2 20 1",
                   "\tscratch_load_dword v5, off, off offset:8 ; 4-byte Folded Reload",
                   "\tscratch_load_dword v6, off, off offset:8 ; 4-byte Folded Reload",
                   "\ts_endpgm", ""])
    p = tmp_path / "g.s"
    p.write_text(g)
    out = subprocess.run([sys.executable, TOOL, str(p), str(p)], check=True, capture_output=True, text=True).stdout
    rows = {l.split()[0]: l.split()[1:] for l in out.split("per source file")[1].split("\n")[2:] if l.strip()}
    assert rows["a.inc"] == ["1", "0"] and rows["b.h"] == ["0", "2"] and rows["total"] == ["1", "2"]
