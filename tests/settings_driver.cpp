// settings_driver.cpp -- prints what outerspace_amd/csrc/osp_settings.h makes of the environment, as one JSON line
// (one key per member of osp::Settings); with --names, the names in its table, one per line with kind and read time.
// Built by tests/test_settings_cpu.py, plain and under AddressSanitizer + UBSan.  Includes nothing else of the library.
#include <cstdio>
#include <cstring>

#include "../outerspace_amd/csrc/osp_settings.h"

using namespace osp;

static void put(const Flag &f) { printf("{\"set\": %s, \"value\": %d}", f.set ? "true" : "false", f.value); }
static void put(const Switch &s) { printf("%s", s.on ? "true" : "false"); }
static void put(const Opt<int> &o) { printf("{\"set\": %s, \"value\": %d}", o.set ? "true" : "false", o.value); }
static void put(const Opt<long> &o) { printf("{\"set\": %s, \"value\": %ld}", o.set ? "true" : "false", o.value); }
static void put(const Opt<uint64_t> &o) { printf("{\"set\": %s, \"value\": %llu}", o.set ? "true" : "false", (unsigned long long)o.value); }
static void put(const Opt<double> &o) { printf("{\"set\": %s, \"value\": \"%a\"}", o.set ? "true" : "false", o.value); }   // (hex float: exact, inf and nan included)
static void put(const Word &w) {
    putchar('"');
    for (char c : w.text) {
        if (c == '"' || c == '\\') putchar('\\');
        putchar(c);
    }
    putchar('"');
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "--names") == 0) {
        static const char *const when[] = {"call", "context", "process"};
#define OSP_X(member, name, Kind, w) printf("%s %s %s\n", name, #Kind, when[w]);
        OSP_SETTINGS(OSP_X)
#undef OSP_X
        return 0;
    }
    const Settings env = Settings::read();
    const char *sep = "{";
#define OSP_X(member, name, Kind, w) printf("%s\"%s\": ", sep, name); put(env.member); sep = ", ";
    OSP_SETTINGS(OSP_X)
#undef OSP_X
    printf("}\n");
    return 0;
}
