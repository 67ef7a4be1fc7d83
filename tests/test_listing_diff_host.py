"""tools/listing_diff.py on hand-written listings: what may differ between two builds of the same kernel (the function index
in labels, .Ltmp numbers, the padding in front of comments, the file a kernel is in) compares equal, and anything else — an
operand, a descriptor line, a kernel that is not there — is reported for that kernel with exit status 1."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "listing_diff.py")


def kernel(name, n, pad, operand="v[2:3]", vgpr=12, tmp=7):
    """A kernel as hipcc -S prints it, as function number n of its file."""
    return "\n".join([
        "\t.globl\t%s" % name,
        "%s:%s; @%s" % (name, pad, name),
        "; %bb.0:",
        "\ts_load_dwordx2 s[2:3], s[0:1], 0x0",
        "\ts_cbranch_execz .LBB%d_2" % n,
        ".Ltmp%d:" % tmp,
        "\tglobal_store_dwordx2 v[0:1], %s, off" % operand,
        ".LBB%d_2:%s; %%bb.2" % (n, pad),
        "\ts_endpgm",
        "\t.amdhsa_kernel %s" % name,
        "\t\t.amdhsa_next_free_vgpr %d" % vgpr,
        "\t.end_amdhsa_kernel",
        ".Lfunc_end%d:" % n,
        "\t.size\t%s, .Lfunc_end%d-%s" % (name, n, name),
        "; NumVgprs: %d" % vgpr,
        ""])


def run(tmp_path, old, *new):
    paths = []
    for i, text in enumerate((old,) + new):
        paths.append(str(tmp_path / ("l%d.s" % i)))
        with open(paths[-1], "w") as f:
            f.write("\t.text\n\t.protected\t__hip_cuid_%dabc\n" % i + text)
    r = subprocess.run([sys.executable, TOOL] + paths, capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout


A, B = "_ZN4heat3k_aEPd", "_ZN4heat3k_bEPdi"
OLD = kernel(A, 0, "    ") + kernel(B, 1, "  ", tmp=8)


def test_renumbered_labels_and_repadded_comments_compare_equal(tmp_path):
    rc, out = run(tmp_path, OLD, kernel(B, 0, "\t\t", tmp=1) + kernel(A, 1, " ", tmp=2))
    assert rc == 0, out
    assert "2 functions identical (2 of them kernels), 0 missing" in out


def test_one_changed_operand_is_reported_for_that_kernel_only(tmp_path):
    rc, out = run(tmp_path, OLD, kernel(A, 0, "    ") + kernel(B, 1, "  ", operand="v[4:5]"))
    assert rc == 1
    assert "DIFFERS: " + B in out and A not in out
    assert "- global_store_dwordx2 v[0:1], v[2:3], off" in out and "+ global_store_dwordx2 v[0:1], v[4:5], off" in out
    assert "1 functions identical (1 of them kernels), 1 missing" in out
    # a descriptor line is part of the kernel
    rc, out = run(tmp_path, OLD, kernel(A, 0, "    ", vgpr=16) + kernel(B, 1, "  "))
    assert rc == 1 and "DIFFERS: " + A in out and "+ .amdhsa_next_free_vgpr 16" in out


def test_a_kernel_in_one_listing_only_is_reported(tmp_path):
    rc, out = run(tmp_path, OLD, kernel(A, 0, "    "))
    assert rc == 1 and "MISSING: " + B in out
    rc, out = run(tmp_path, kernel(A, 0, "    "), OLD)
    assert rc == 1 and "ADDED  : " + B in out
    assert "1 functions identical (1 of them kernels), 1 missing" in out


def test_a_kernel_moved_to_the_second_new_listing_compares_equal(tmp_path):
    rc, out = run(tmp_path, OLD, kernel(A, 0, "    "), kernel(B, 0, "  ", tmp=0))
    assert rc == 0, out
    assert "2 functions identical (2 of them kernels), 0 missing" in out
