// merge_host.cpp -- sambamba_amd/csrc/merge_core.hpp on the CPU (tests/test_merge_core_cpu.py): the header merge of sbx_merge_bam
// through the very function the library compiles.
//   merge_host FILE...   every FILE holds one header text, in input order.  Prints "rc <code>"; after a refusal "why <message>";
//                        otherwise "sq <name>:<length>,..." , per input "ref <input> <new id>,...", "rg <input> <old>\t<new>" and
//                        "pg <input> <old>\t<new>" per merged line, then "text" and the merged header text up to the end of the output.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "../../sambamba_amd/csrc/merge_core.hpp"

int main(int argc, char** argv) {
    std::vector<std::string> texts;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        std::stringstream ss;
        ss << f.rdbuf();
        texts.push_back(ss.str());
    }
    sbx::mergec::MergedHeader m;
    std::string why;
    const int rc = sbx::mergec::merge_headers(texts, &m, &why);
    printf("rc %d\n", rc);
    if (rc != SBX_OK) { printf("why %s\n", why.c_str()); return 0; }
    printf("sq ");
    for (size_t k = 0; k < m.refs.size(); ++k) printf("%s%s:%d", k ? "," : "", m.refs[k].name.c_str(), m.refs[k].length);
    printf("\n");
    for (size_t f = 0; f < m.maps.size(); ++f) {
        printf("ref %zu ", f);
        for (size_t k = 0; k < m.maps[f].ref.size(); ++k) printf("%s%d", k ? "," : "", m.maps[f].ref[k]);
        printf("\n");
        for (const auto& e : m.maps[f].rg) printf("rg %zu %s\t%s\n", f, e.first.c_str(), e.second.c_str());
        for (const auto& e : m.maps[f].pg) printf("pg %zu %s\t%s\n", f, e.first.c_str(), e.second.c_str());
    }
    printf("text\n");
    fwrite(m.text.data(), 1, m.text.size(), stdout);
    return 0;
}
