"""tools/isa_diff.py: the kernel-by-kernel comparison of two builds (instruction text and the
register / LDS / scratch figures of the kernel metadata).  Synthetic listings check that equal
builds pass and that each kind of difference is found.  CPU only."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_diff  # noqa: E402

K1, K2 = "_ZN2rr6k_testEv", "_ZN2rr7k_otherEv"


def dis(kernels, base=0x1000):
    """{symbol: [instruction]} -> llvm-objdump -d lines"""
    out = ["", "g.co:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""]
    for i, (k, ins) in enumerate(kernels.items()):
        addr = base + 0x100 * i
        out.append("%016x <%s>:" % (addr, k))
        out += ["\t%s      // %012X: 00000000" % (x, addr + 4 * j) for j, x in enumerate(ins)]
        out.append("")
    return out


def notes(kernels):
    """{symbol: (vgpr, sgpr, lds, scratch)} -> llvm-readelf --notes lines"""
    out = ["Displaying notes found in: .note", "    AMDGPU Metadata:", "        ---", "amdhsa.kernels:"]
    for k, (v, s, lds, scr) in kernels.items():
        out += ["  - .agpr_count:     0", "    .args:", "      - .offset:         0", "        .size:           176",
                "        .value_kind:     by_value", "    .group_segment_fixed_size: %d" % lds,
                "    .kernarg_segment_align: 8", "    .language_version:", "      - 2", "      - 0",
                "    .name:           %s" % k, "    .private_segment_fixed_size: %d" % scr,
                "    .sgpr_count:     %d" % s, "    .sgpr_spill_count: 0", "    .symbol:         %s.kd" % k,
                "    .vgpr_count:     %d" % v, "    .vgpr_spill_count: 0", "    .wavefront_size: 64"]
    out += ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2", "..."]
    return out


INS = {K1: ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "s_endpgm"],
       K2: ["v_mov_b32_e32 v1, 0", "s_cbranch_scc0 6", "s_endpgm"]}
MD = {K1: (64, 32, 65536, 0), K2: (128, 48, 0, 0)}


def verdicts(ins_a, md_a, ins_b, md_b, **kw):
    rows = isa_diff.compare(isa_diff.functions(dis(ins_a)), isa_diff.metadata(notes(md_a)),
                            isa_diff.functions(dis(ins_b, **kw)), isa_diff.metadata(notes(md_b)))
    return dict(rows)


def test_parsers_read_the_listings():
    assert isa_diff.functions(dis(INS)) == INS
    assert isa_diff.metadata(notes(MD))[K2] == {".vgpr_count": "128", ".sgpr_count": "48",
                                                ".group_segment_fixed_size": "0", ".private_segment_fixed_size": "0"}


def test_equal_listings_pass_wherever_the_kernels_sit():
    v = verdicts(INS, MD, INS, MD, base=0x7300)   # other addresses: a kernel may move inside its object
    assert v == {K1: "same", K2: "same"}


def test_changed_instruction_is_found():
    ins = dict(INS, **{K2: ["v_mov_b32_e32 v1, 0", "s_cbranch_scc0 7", "s_endpgm"]})
    v = verdicts(INS, MD, ins, MD)
    assert v[K1] == "same" and "instruction 1" in v[K2] and "s_cbranch_scc0 7" in v[K2]
    longer = dict(INS, **{K1: INS[K1][:2] + ["s_nop 0", "s_endpgm"]})
    assert "instruction 2 of 3 / 4" in verdicts(INS, MD, longer, MD)[K1]


def test_changed_register_count_is_found():
    for i, field in enumerate(isa_diff.META):
        vals = {".vgpr_count": 0, ".sgpr_count": 1, ".group_segment_fixed_size": 2, ".private_segment_fixed_size": 3}
        t = list(MD[K1])
        t[vals[field]] += 8
        v = verdicts(INS, MD, INS, dict(MD, **{K1: tuple(t)}))
        assert field in v[K1] and v[K2] == "same"


def test_missing_kernel_is_found():
    v = verdicts(INS, MD, {K1: INS[K1]}, {K1: MD[K1]})
    assert v[K1] == "same" and v[K2] == "only in the old build"
    v = verdicts({K1: INS[K1]}, {K1: MD[K1]}, INS, MD)
    assert v[K2] == "only in the new build"
    # a function that lost its kernel descriptor
    assert "metadata on one side" in verdicts(INS, MD, INS, {K1: MD[K1]})[K2]
