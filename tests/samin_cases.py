"""The SAM lines the import tests share (tests/test_samin_core_cpu.py on the CPU, tests/test_gpu_import.py on the device): every field
at both ends of its range, every tag type, and one line per rule of the grammar that it breaks.  The references are those of
tests/sam_cases.py."""
import struct

from tests.sam_cases import REF_NAMES, REFS, TEXT  # noqa: F401

TAIL = b"\tc1\t100\t30\t4M\t=\t200\t50\tACGT\tIIII"


def line(name=b"r", flag=b"0", rname=b"c1", pos=b"100", mapq=b"30", cigar=b"4M", rnext=b"=", pnext=b"200", tlen=b"50", seq=b"ACGT", qual=b"IIII",
         tags=()):
    return b"\t".join([name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(tags))


def good_lines():
    """{case: line}, in a fixed order"""
    g = {}
    g["plain"] = line()
    g["unmapped"] = line(b"r1", b"0", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"*", b"*")
    g["hand"] = line(b"q", b"99", b"c2", b"17000", b"60", b"2M1D2M", b"=", b"17100", b"-150", b"ACGT", b"!~I*", [b"NM:i:-1", b"XA:A:x"])
    # QNAME: '*', a name that starts with '*', both ends of the class, 254 bytes
    g["qname_star"] = line(b"*")
    g["qname_star_first"] = line(b"*abc")
    g["qname_class_ends"] = line(b"!?A~")
    g["qname_254"] = line(b"N" * 254)
    # FLAG, MAPQ, POS, PNEXT, TLEN at both ends; 18 digits
    g["flag_mapq_max"] = line(flag=b"65535", mapq=b"255")
    g["flag_18_digits"] = line(flag=b"000000000000065535", mapq=b"000000000000000000")
    g["pos_0"] = line(pos=b"0", pnext=b"0")
    g["pos_0_unmapped_cigar"] = line(rname=b"*", pos=b"0", cigar=b"*", rnext=b"*", pnext=b"0")
    g["pos_max"] = line(pos=b"2147483647", pnext=b"2147483647", cigar=b"*")
    g["pos_max_cigar"] = line(pos=b"2147483647", cigar=b"4M")          # (the end wraps as the reference's int does)
    g["tlen_min"] = line(tlen=b"-2147483648")
    g["tlen_max"] = line(tlen=b"2147483647")
    g["tlen_plus"] = line(tlen=b"+5")
    # RNAME / RNEXT
    g["rnext_star"] = line(rnext=b"*")
    g["rnext_other"] = line(rnext=b"chrWithALongerName_3")
    g["rname_star_rnext_eq"] = line(rname=b"*", rnext=b"=")
    g["rname_star_rnext_name"] = line(rname=b"*", rnext=b"c2")
    g["rname_last"] = line(rname=b"chrWithALongerName_3")
    # CIGAR
    g["cigar_star"] = line(cigar=b"*")
    g["cigar_all_ops"] = line(cigar=b"1M2I3D4N5S6H7P8=9X")
    g["cigar_longest_op"] = line(cigar=b"268435455S1M")
    g["cigar_span_levels"] = line(pos=b"16384", cigar=b"1M200000N3M")
    g["cigar_18_digits"] = line(cigar=b"000000000000000004M")
    g["cigar_no_reference"] = line(cigar=b"4I")
    g["cigar_65535"] = line(name=b"cigmax", cigar=b"".join(b"%d%c" % (k % 1000 + 1, b"MIDNSHP=X"[k % 9]) for k in range(65535)))
    # SEQ: both sides of the 8-byte store, every character of the class
    for n in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255):
        s = bytes(b"ACGTNacgtn=.RYKMSWBDHVrykmswbdhvXZxz"[k % 36] for k in range(n))
        g["seq_%d" % n] = line(name=b"seq%03d" % n, cigar=b"*", seq=s, qual=bytes(33 + (7 * k) % 94 for k in range(n)))
    g["seq_every_letter"] = line(cigar=b"*", seq=bytes(range(65, 91)) + bytes(range(97, 123)) + b"=.", qual=b"5" * 54)
    # QUAL: the three '*' cases, both ends of the class
    g["qual_star_no_seq"] = line(cigar=b"*", seq=b"*", qual=b"*")
    g["qual_star_one_base"] = line(cigar=b"*", seq=b"A", qual=b"*")
    g["qual_star_bases"] = line(cigar=b"*", seq=b"ACGTA", qual=b"*")
    g["qual_class_ends"] = line(qual=b"!~!~")
    # tags
    g["tag_A"] = line(tags=[b"XA:A:!", b"XB:A:~", b"x9:A:A"])
    ints = [0, 5, 127, 128, 255, 256, 65535, 65536, 2147483647, 2147483648, 4294967295, -1, -128, -129, -32768, -32769, -2147483648]
    g["tag_i_borders"] = line(tags=[b"I%c:i:%d" % (65 + k, v) for k, v in enumerate(ints)])
    g["tag_i_signs"] = line(tags=[b"Xa:i:-0", b"Xb:i:+5", b"Xc:i:+0", b"Xd:i:000000000000000042", b"Xe:i:-000000000000000300"])
    floats = [b"1", b"-0", b".5", b"0.1", b"1e39", b"-1e39", b"1e-46", b"-1e-46", b"inf", b"+inf", b"-inf", b"nan", b"-nan", b"3.4028235e38",
              b"3.4028236e38", b"1.4e-45", b"7.006492321624085e-46", b"7.006492321624086e-46", b"16777217", b"16777217.0000000000000000000001",
              b"16777219", b"1E5", b"1e+5", b"+1.5e-3", b"00012.500", b"1e00000000000000000000000000005", b"0e999999999999",
              b"1.17549435e-38", b"1.1754942e-38", b"340282356779733661637539395458142568448", b"340282356779733661637539395458142568447.9"]
    g["tag_f"] = line(tags=[b"F%c:f:%s" % (48 + k if k < 10 else 55 + k, v) for k, v in enumerate(floats)])
    g["tag_Z_H"] = line(tags=[b"Z0:Z: ", b"Z1:Z:x y~!", b"Z2:Z:" + b"z" * 700, b"H0:H:0", b"H1:H:1AE3f", b"H2:H:" + b"9aF" * 99])
    g["tag_B_borders"] = line(tags=[b"Bc:B:c,-128,127,+0", b"BC:B:C,0,255", b"Bs:B:s,-32768,32767", b"BS:B:S,0,65535", b"Bi:B:i,-2147483648,2147483647",
                                    b"BI:B:I,0,4294967295", b"Bf:B:f,1.5,-nan,inf,-0,1e-46,1e39"])
    g["tag_B_empty"] = line(tags=[b"B0:B:c,", b"B1:B:f,", b"B2:B:I,"])
    g["tag_B_nine"] = line(tags=[b"B9:B:s," + b",".join(b"%d" % ((-1) ** k * 7 * k) for k in range(9))])
    g["tags_forty"] = line(tags=[b"%c%c:i:%d" % (65 + k // 10, 48 + k % 10, k * 1000) for k in range(40)])
    return g


# the records of three of the lines, written out by hand
HAND = {
    "unmapped": struct.pack("<iiiBBHHHiiii", 35, -1, -1, 3, 0, 4680, 0, 0, 0, -1, -1, 0) + b"r1\0",
    # c2 is reference 1; POS 17000 and five reference bases end at 17004 (0-based), both in the 16 KiB window 1: bin 4681 + 1
    "hand": struct.pack("<iiiBBHHHiiii", 32 + 2 + 12 + 2 + 4 + 4 + 4, 1, 16999, 2, 60, 4682, 3, 99, 4, 1, 17099, -150) + b"q\0" +
            struct.pack("<III", 2 << 4, 1 << 4 | 2, 2 << 4) + b"\x12\x48" + bytes([0, 93, 40, 9]) + b"NMc\xff" + b"XAAx",
    "qual_star_bases": struct.pack("<iiiBBHHHiiii", 32 + 2 + 3 + 5, 0, 99, 2, 30, 4681, 0, 0, 5, 0, 199, 50) + b"r\0" + b"\x12\x48\x10" + b"\xff" * 5,
}


def malformed_lines():
    """{case: line}: one line per rule, each breaking that rule alone"""
    b = {}
    b["empty_line"] = b""
    b["ten_fields"] = b"\t".join(line().split(b"\t")[:10])
    b["at_line"] = line(b"@CO")
    b["cr_at_end"] = line() + b"\r"
    b["cr_inside"] = line(tags=[b"XZ:Z:a\rb"])
    b["trailing_tab"] = line() + b"\t"
    b["qname_empty"] = line(b"")
    b["qname_255"] = line(b"N" * 255)
    b["qname_space"] = line(b"a b")
    b["flag_65536"] = line(flag=b"65536")
    b["flag_19_digits"] = line(flag=b"0000000000000000001")
    b["flag_empty"] = line(flag=b"")
    b["flag_signed"] = line(flag=b"+4")
    b["mapq_256"] = line(mapq=b"256")
    b["pos_2_31"] = line(pos=b"2147483648")
    b["pos_negative"] = line(pos=b"-1")
    b["pnext_2_31"] = line(pnext=b"2147483648")
    b["tlen_2_31"] = line(tlen=b"2147483648")
    b["tlen_below_min"] = line(tlen=b"-2147483649")
    b["tlen_bare_sign"] = line(tlen=b"-")
    b["rname_unknown"] = line(rname=b"c3")
    b["rname_star_more"] = line(rname=b"*x")
    b["rname_equals"] = line(rname=b"=")
    b["rname_empty"] = line(rname=b"")
    b["rnext_unknown"] = line(rnext=b"c3")
    b["rnext_equals_more"] = line(rnext=b"=c1")
    b["cigar_bad_op"] = line(cigar=b"4Z")
    b["cigar_no_length"] = line(cigar=b"M")
    b["cigar_2_28"] = line(cigar=b"268435456M")
    b["cigar_19_digits"] = line(cigar=b"0000000000000000004M")
    b["cigar_trailing_digits"] = line(cigar=b"4M5")
    b["cigar_empty"] = line(cigar=b"")
    b["cigar_star_more"] = line(cigar=b"*4M")
    b["cigar_65536"] = line(cigar=b"1M" * 65536)
    b["seq_bad_char"] = line(seq=b"AC-T")
    b["seq_empty"] = line(seq=b"")
    b["seq_star_more"] = line(seq=b"*CGT")
    b["qual_short"] = line(qual=b"III")
    b["qual_long"] = line(qual=b"IIIII")
    b["qual_space"] = line(qual=b"II I")
    b["qual_empty"] = line(qual=b"")
    b["qual_for_no_seq"] = line(cigar=b"*", seq=b"*", qual=b"II")
    b["tag_short_key"] = line(tags=[b"X:i:1"])
    b["tag_key_digit_first"] = line(tags=[b"1X:i:1"])
    b["tag_unknown_type"] = line(tags=[b"XX:Q:1"])
    b["tag_no_value"] = line(tags=[b"XX:i:"])
    b["tag_A_two_bytes"] = line(tags=[b"XX:A:ab"])
    b["tag_A_space"] = line(tags=[b"XX:A: "])
    b["tag_i_19_digits"] = line(tags=[b"XX:i:1000000000000000000"])
    b["tag_i_2_32"] = line(tags=[b"XX:i:4294967296"])
    b["tag_i_below_int_min"] = line(tags=[b"XX:i:-2147483649"])
    b["tag_i_letters"] = line(tags=[b"XX:i:zzz"])
    b["tag_f_point_at_end"] = line(tags=[b"XX:f:1."])
    b["tag_f_plus_nan"] = line(tags=[b"XX:f:+nan"])
    b["tag_f_upper_inf"] = line(tags=[b"XX:f:INF"])
    b["tag_f_bare_exponent"] = line(tags=[b"XX:f:1e"])
    b["tag_Z_control"] = line(tags=[b"XX:Z:a\x01b"])
    b["tag_H_not_hex"] = line(tags=[b"XX:H:12G4"])
    b["tag_B_unknown_type"] = line(tags=[b"XX:B:x,1"])
    b["tag_B_no_comma"] = line(tags=[b"XX:B:c"])
    b["tag_B_c_128"] = line(tags=[b"XX:B:c,127,128"])
    b["tag_B_C_negative"] = line(tags=[b"XX:B:C,-1"])
    b["tag_B_S_65536"] = line(tags=[b"XX:B:S,65536"])
    b["tag_B_I_2_32"] = line(tags=[b"XX:B:I,4294967296"])
    b["tag_B_empty_element"] = line(tags=[b"XX:B:c,1,,2"])
    b["tag_B_comma_at_end"] = line(tags=[b"XX:B:c,1,"])
    b["tag_B_float_in_ints"] = line(tags=[b"XX:B:i,1.5"])
    b["second_tag_bad"] = line(tags=[b"X1:i:7", b"X3:i:zzz", b"X4:i:5"])
    return b


def sam_text(lines, final_newline=True):
    body = b"\n".join(lines) + (b"\n" if final_newline and lines else b"")
    return TEXT.encode() + body
