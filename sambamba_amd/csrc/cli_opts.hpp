// cli_opts.hpp -- the one argument scanner of sbx-depth, sbx-sort, sbx-flagstat and sbx-markdup.  It knows the forms D's getopt knows --
// `--name=value`, `--name value`, `-Xvalue`, `-X=value`, `-X value`, options before or after the file names -- and classifies ONE
// argument at a time.  It decides nothing: what an unknown option, a `--` or a flag with text attached MEANS is the policy of each
// command line, stated where its loop handles the token.
#pragma once
#include <string>

namespace sbx {

struct OptSpec { const char* lng; char sht; bool takes_value; int id; };     // sht == 0: no short form
struct OptToken {
    enum Kind { Option, Positional, Unknown, Terminator } kind = Positional;
    const OptSpec* spec = nullptr;   // Option: which one
    std::string arg;                 // the argument as written
    std::string value;               // Option: the attached text, or the following argument of an option that takes a value
    bool attached = false;           // ... text was attached (`--name=text`, `-Xtext`, `-X=text`), to a flag as well
    bool missing = false;            // ... the option takes a value and was the last argument
};

// Classifies argv[*i]; an option that takes a value and has none attached consumes argv[*i + 1] (then *i is advanced).
// `--` alone is the Terminator, `--x...` / `-x...` that no spec names are Unknown, everything else (a lone `-` too) is Positional.
template <size_t N> OptToken next_opt(int argc, char** argv, int* i, const OptSpec (&specs)[N]) {
    OptToken t;
    const std::string& a = t.arg = argv[*i];
    if (a == "--") { t.kind = OptToken::Terminator; return t; }
    if (a.size() < 2 || a[0] != '-') return t;
    t.kind = OptToken::Unknown;
    if (a[1] == '-') {
        const size_t eq = a.find('=');
        const std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
        for (const OptSpec& s : specs) if (name == s.lng) t.spec = &s;
        if (eq != std::string::npos) { t.value = a.substr(eq + 1); t.attached = true; }
    } else {
        for (const OptSpec& s : specs) if (s.sht && a[1] == s.sht) t.spec = &s;
        if (a.size() > 2) { t.value = a.substr(a[2] == '=' ? 3 : 2); t.attached = true; }
    }
    if (!t.spec) return t;
    t.kind = OptToken::Option;
    if (t.spec->takes_value && !t.attached) {
        if (*i + 1 >= argc) t.missing = true;
        else t.value = argv[++*i];
    }
    return t;
}

}  // namespace sbx
