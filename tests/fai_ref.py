"""`sambamba index -F` restated in Python from its semantics (buildFai, BioD bio/std/file/fai.d:78-101), with the three deliberate
divergences of sbx_index_fasta: an empty file gives an empty index, a first line that is no header is refused, and with "\\r\\n" a
'\\n' without '\\r' in front of it is refused with the count and the number of the first such line.  Also the inputs the CPU and the
GPU tests share."""
import random


class SequenceBeforeHeader(Exception):
    pass


class BareNewline(Exception):
    def __init__(self, count, first_line):
        super().__init__("%d bare line ends, the first ends line %d" % (count, first_line))
        self.count = count
        self.first_line = first_line


def terminator(data):
    k = data.find(b"\n")
    return b"\r\n" if k > 0 and data[k - 1:k] == b"\r" else b"\n"


def lines_of(data, term):
    """split at the terminator only; a last line without terminator is a line, a text that ends in it has no extra empty line"""
    lines = data.split(term)
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def fai(data):
    """the text of the .fai of `data` (bytes)"""
    if not data:
        return b""
    term = terminator(data)
    if not data.startswith(b">"):
        raise SequenceBeforeHeader()
    lines = lines_of(data, term)
    if term == b"\r\n":
        bare = [k + 1 for k, l in enumerate(lines) if b"\n" in l]
        if bare:
            # every bare '\n' ends a line of its own in the count and in the numbering
            count, number, first = 0, 0, None
            for l in lines:
                for _ in range(l.count(b"\n")):
                    number += 1
                    count += 1
                    if first is None:
                        first = number
                number += 1
            raise BareNewline(count, first)
    records = []
    offset = 0
    for line in lines:
        offset += len(line) + len(term)
        if line.startswith(b">"):
            records.append({"name": line.split(b" ")[0][1:], "seq_len": 0, "offset": offset, "line_len": 0})
        else:
            r = records[-1]
            if r["line_len"] == 0:
                r["line_len"] = len(line)
            r["seq_len"] += len(line)
    return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % (r["name"], r["seq_len"], r["offset"], r["line_len"], r["line_len"] + len(term)) for r in records)


def complaint(path, exc):
    """the message of sbx_index_fasta for the refusal `exc`"""
    if isinstance(exc, SequenceBeforeHeader):
        return "malformed FASTA text in %s: line 1 does not start with '>' (sequence in front of the first header)" % path
    return ("malformed FASTA text in %s: %d %s in '\\n' without '\\r' though the first line ends in \"\\r\\n\", the first is line %d"
            % (path, exc.count, "line ends" if exc.count == 1 else "lines end", exc.first_line))


GOLDEN_FAI = b"one\t66\t5\t30\t31\ntwo\t28\t98\t14\t15\n"

# name -> text; the chunk sizes of the tests (16, 32, 48, 4096, whole) cut them at many places
CASES = {
    "crlf": b">a\r\nAC\r\nG\r\n",
    "last_line_open": b">a\nACGT\nAC",
    "last_line_open_header": b">a\nACGT\n>b x",
    "empty_first_sequence_line": b">a\n\nACGT\nAC\n",
    "empty_name": b">\nACGT\n",
    "empty_name_space": b"> x\nACGT\n",
    "tab_in_header": b">a\tb c\nACGT\n",
    "header_longer_than_a_chunk": b">" + b"n" * 70 + b" " + b"d" * 50 + b"\nACGT\nAC\n>" + b"m" * 100 + b"\nAC\n",
    "line_longer_than_several_chunks": b">a\n" + b"ACGT" * 60 + b"\n" + b"AC" * 10 + b"\n>b\n" + b"G" * 333 + b"\n",
    "cr_at_chunk_end": b">abcdefghijklmn\r\nAC\r\n" + b"ACGTACGTAC\r\n" * 5 + b">b\r\nA\r\n",      # the '\r' of line 1 is byte 15
    "cr_in_lf_file": b">a\nAC\rGT\nAC\r\n\r\n",
    "crlf_open_end_cr": b">a\r\nAC\r\nAC\r",
    "crlf_empty_lines": b">a\r\n\r\nAC\r\n\r\n",
    "only_header": b">a",
    "only_header_nl": b">a\n",
    "many_headers": b"".join(b">s%d d\nAC\n" % k for k in range(40)),
    "blank_lines_everywhere": b">a\n\n\n\nAC\n\n>b\n\n",
    "empty": b"",
}
ERRORS = {
    "sequence_first": b"ACGT\n>a\nAC\n",
    "blank_first": b"\n>a\nAC\n",
    "bare_newline": b">a\r\nAC\nGT\r\nA\nC\n\nG\r\n",
    "bare_newline_one": b">a\r\nACGTACGTACGTACGTACGT\r\nGT\nAC\r\n",
}


def random_case(rng):
    """a small FASTA text: a few records, wrapped at random widths, sometimes CRLF, ragged ends, empty lines, spaces in headers"""
    term = b"\r\n" if rng.random() < 0.3 else b"\n"
    out = []
    for _ in range(rng.randint(1, 5)):
        name = bytes(rng.choice(b"abcXYZ_01\t") for _ in range(rng.randint(0, 12)))
        if rng.random() < 0.4:
            name += b" " + bytes(rng.choice(b"desc >") for _ in range(rng.randint(0, 30)))
        out.append(b">" + name)
        width = rng.choice((1, 3, 7, 15, 16, 17, 31, 60))
        for _ in range(rng.randint(0, 6)):
            r = rng.random()
            out.append(b"" if r < 0.1 else bytes(rng.choice(b"ACGTN\r" if term == b"\n" else b"ACGTN") for _ in range(width if r < 0.8 else rng.randint(1, width))))
    text = term.join(out)
    if rng.random() < 0.7:
        text += term
    return text


def random_cases(seed=20241019, n=300):
    rng = random.Random(seed)
    return [random_case(rng) for _ in range(n)]


def expected(data):
    """("ok", fai text) or ("seq",) or ("bare", count, first line)"""
    try:
        return ("ok", fai(data))
    except SequenceBeforeHeader:
        return ("seq",)
    except BareNewline as e:
        return ("bare", e.count, e.first_line)
