// entry_host.cpp -- sambamba_amd/csrc/entry_util.hpp on the CPU (tests/test_entry_util_cpu.py): the host-only helpers of the standalone
// entry points, through the very functions the library compiles, built with -fsanitize=address,undefined.  No device, no HIP.
//   entry_host DIR   runs every check in the (empty, writable) directory DIR; prints "ok" and exits 0, or names the first failure
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../sambamba_amd/csrc/entry_util.hpp"

using namespace sbx;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static bool exists(const std::string& p) { return access(p.c_str(), F_OK) == 0; }
static void touch(const std::string& p) { FILE* f = fopen(p.c_str(), "wb"); if (f) { fputs("x", f); fclose(f); } }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];

    // ---- copy_to_caller: the buffer is exactly as long as the caller says (heap, so that the sanitizer sees an overrun) ----
    {
        const std::string t = "hello";
        size_t len = 99;
        char* buf = (char*)malloc(6);
        CHECK(copy_to_caller(t, buf, 6, &len) == SBX_OK && len == 5 && std::string(buf) == "hello");
        memset(buf, '#', 6);
        len = 99;
        CHECK(copy_to_caller(t, buf, 5, &len) == SBX_ENOMEM && len == 5 && buf[0] == '#' && buf[5] == '#');     // no room for the NUL: untouched
        CHECK(copy_to_caller(t, buf, 0, &len) == SBX_ENOMEM && buf[0] == '#');
        CHECK(copy_to_caller(t, nullptr, 100, &len) == SBX_ENOMEM && len == 5);
        CHECK(copy_to_caller(t, buf, 6, nullptr) == SBX_OK);
        // a message handed out with its code: the code comes back when it fits, and when it does not
        CHECK(copy_to_caller(t, buf, 6, &len, SBX_EFORMAT) == SBX_EFORMAT && std::string(buf) == "hello");
        CHECK(copy_to_caller(t, buf, 2, &len, SBX_EFORMAT) == SBX_EFORMAT && len == 5);
        free(buf);
        char one[1] = {'#'};
        CHECK(copy_to_caller("", one, 1, &len) == SBX_OK && len == 0 && one[0] == 0);
    }

    // ---- malformed_records_message ----
    CHECK(malformed_records_message(3) ==
          "malformed BAM record (3 records whose reference id is out of range or whose lengths are inconsistent)");
    CHECK(malformed_records_message(1, "a b.bam") ==
          "malformed BAM record in a b.bam (1 records whose reference id is out of range or whose lengths are inconsistent)");
    CHECK(malformed_records_message(18446744073709551615ull).find("(18446744073709551615 records") != std::string::npos);

    // ---- OutputGuard: unlink unless disarmed, never before armed, never for stdout ----
    {
        const std::string a = dir + "/armed.bam", b = dir + "/disarmed.bam", c = dir + "/never_armed.bam", d = dir + "/stdout.bam";
        touch(a); touch(b); touch(c); touch(d);
        { OutputGuard g(a.c_str()); g.arm(); CHECK(g.armed && std::string(g.c_str()) == a); }
        CHECK(!exists(a));
        { OutputGuard g(b.c_str()); g.arm(); g.disarm(); }
        CHECK(exists(b));
        { OutputGuard g(c.c_str()); }
        CHECK(exists(c));
        { OutputGuard g(d.c_str(), true); g.arm(); CHECK(!g.armed); }
        CHECK(exists(d));
        { OutputGuard g((dir + "/absent.bam").c_str()); g.arm(); }              // nothing to remove: no error
        try { OutputGuard g(b.c_str()); g.arm(); throw 1; } catch (int) {}        // unwinding removes it
        CHECK(!exists(b));
        { OutputGuard g(nullptr); g.arm(); }
    }

    // ---- same_file ----
    {
        const std::string a = dir + "/x.bam", l = dir + "/x.link";
        touch(a);
        CHECK(same_file(a.c_str(), a.c_str()) && same_file(a.c_str(), (dir + "/./x.bam").c_str()));
        CHECK(symlink(a.c_str(), l.c_str()) == 0 && same_file(a.c_str(), l.c_str()));
        CHECK(!same_file(a.c_str(), (dir + "/never_armed.bam").c_str()) && !same_file(a.c_str(), (dir + "/absent").c_str()));
    }

    // ---- env_u64: a plain decimal number, or nothing ----
    {
        const char* const name = "SBX_ENTRY_HOST_HOOK";
        auto with = [&](const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); return env_u64(name); };
        CHECK(!with(nullptr) && !with("") && !with("12x") && !with("-1") && !with(" 5") && !with("+5") && !with("x") && !with("5 "));
        CHECK(with("0") && *with("0") == 0);
        CHECK(with("65280") == std::optional<uint64_t>(65280) && with("007") == std::optional<uint64_t>(7));
        CHECK(with("18446744073709551615") == std::optional<uint64_t>(18446744073709551615ull));
        // What the six hooks make of it -- unset, "0", an ordinary number -- as the arithmetic their one-liners put on env_u64 / env_size:
        // the two window hooks (0 stands for unset), the SAM piece and the import chunk (64 MiB unless at least 1), the FASTA chunk (64 MiB
        // unless at least 16; down to a multiple of 16; at most fastac::kChunkLimit = 1 GiB), the BGZF piece (into [1, kBgzfPieceBlocks = 32768]).
        const uint64_t k64M = 64ull << 20, kLimit = 1ull << 30, kPiece = 32768;
        auto window_hook = [&] { return env_u64(name).value_or(0); };
        auto chunk = [&] { return env_size(name, k64M); };
        auto fasta = [&] { return std::min<uint64_t>(env_size(name, k64M, 16) & ~15ull, kLimit); };
        auto piece = [&] { return std::min<uint64_t>(std::max<uint64_t>(env_u64(name).value_or(kPiece), 1), kPiece); };
        with(nullptr);
        CHECK(window_hook() == 0 && chunk() == k64M && fasta() == k64M && piece() == kPiece);
        with("0");
        CHECK(window_hook() == 0 && chunk() == k64M && fasta() == k64M && piece() == 1);
        with("65281");
        CHECK(window_hook() == 65281 && chunk() == 65281 && fasta() == 65280 && piece() == kPiece);
        with("15");
        CHECK(chunk() == 15 && fasta() == k64M && piece() == 15);
        with("16");
        CHECK(fasta() == 16);
        with("18446744073709551615");
        CHECK(window_hook() == ~0ull && chunk() == ~0ull && fasta() == kLimit && piece() == kPiece);
        with("12x");
        CHECK(window_hook() == 0 && chunk() == k64M && fasta() == k64M && piece() == kPiece);
        CHECK(env_size(name, 7, 3) == 7);
        with("2");
        CHECK(env_size(name, 7, 3) == 7 && env_size(name, 7, 2) == 2);
        unsetenv(name);
    }

    // ---- OutputFile: the file of a command, written piece by piece ----
    {
        auto slurp = [](const std::string& p) { std::string s; FILE* f = fopen(p.c_str(), "rb"); if (f) { char b[256]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) s.append(b, k); fclose(f); } return s; };
        // finished with the EOF block: the bytes written, then its 28; the guard was armed when the file came to be and still is
        const std::string a = dir + "/sink_eof.bam";
        {
            OutputGuard g(a.c_str());
            OutputFile f(g);
            CHECK(g.armed && exists(a) && f.ok());
            f.write("abc", 3);
            f.write("", 0);
            f.write("de", 2);
            f.finish(true);
            CHECK(g.armed && f.ok());
            const std::string got = slurp(a);
            CHECK(got.size() == 5 + 28 && got.compare(0, 5, "abcde") == 0 && memcmp(got.data() + 5, kEofBlock, 28) == 0);
            CHECK(kEofBlock[0] == 0x1f && kEofBlock[1] == 0x8b && kEofBlock[16] == 0x1b && kEofBlock[27] == 0);
        }
        CHECK(!exists(a));                                   // (the guard died armed)
        // finished without it: exactly what was written; no guard: nothing removes the file
        const std::string b = dir + "/sink_plain.sam";
        { OutputFile f(b); f.write("line\n", 5); f.finish(false); }
        CHECK(slurp(b) == "line\n");
        { OutputFile f(b); f.finish(false); }               // "wb": an existing file is cut
        CHECK(exists(b) && slurp(b).empty());
        // a directory that is not there: SBX_EIO "cannot write", nothing created, the guard not armed
        const std::string c = dir + "/no_such_dir/out.bam";
        {
            OutputGuard g(c.c_str());
            int code = 0;
            std::string what;
            try { OutputFile f(g); } catch (const Error& e) { code = e.code; what = e.what(); }
            CHECK(code == SBX_EIO && what == "cannot write " + c && !g.armed);
        }
        CHECK(!exists(c) && !exists(dir + "/no_such_dir"));
        // destroyed without finish() (an exception passes by): the file is closed -- no leak under the sanitizer -- and the armed guard removes it
        const std::string d = dir + "/sink_unfinished.bam";
        try {
            OutputGuard g(d.c_str());
            OutputFile f(g);
            f.write("xyz", 3);
            CHECK(exists(d));
            throw 1;
        } catch (int) {}
        CHECK(!exists(d));
        // a write that fails is latched and finish() says so: /dev/full takes no byte
        if (exists("/dev/full")) {
            int code = 0;
            std::string what;
            try {
                OutputFile f("/dev/full");
                std::string big(1 << 20, 'x');
                f.write(big.data(), big.size());
                f.write("a", 1);
                f.finish(true);
            } catch (const Error& e) { code = e.code; what = e.what(); }
            CHECK(code == SBX_EIO && what == "error writing /dev/full");
        }
    }
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
