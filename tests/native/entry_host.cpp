// entry_host.cpp -- sambamba_amd/csrc/entry_util.hpp on the CPU (tests/test_entry_util_cpu.py): the host-only helpers of the standalone
// entry points, through the very functions the library compiles, built with -fsanitize=address,undefined.  No device, no HIP.
//   entry_host DIR   runs every check in the (empty, writable) directory DIR; prints "ok" and exits 0, or names the first failure
#include <cstdio>
#include <cstdlib>
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
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
