// jit_dump — csrc/jit_gen.cpp on its own (host only: g++ on graph.cpp + approx.cpp + flatten.cpp + srk.cpp + jit_gen.cpp, no HIP): loads
// rack files, flattens each for a voice count and render flags the way a diagnostic call of the library does (no per-voice overrides: a
// rack file carries none), and prints a digest of the generated kernel text for every combination of output mode 1 .. 4, without / with
// the control units, and want_waves 0 / 2 / 4 — or, with --text, the text of one combination.  tests/test_jit_gen_host.py drives it.
//   jit_dump [--voices V] [--flags F] [--buffer B] [--text [--mode M] [--ctl 0|1|auto] [--waves W]] file.srk ...
// Options apply to the files after them.  A line per result:  <file> mode=M ctl=C waves=W <fnv-1a digest> <bytes>   or   ... error: <message>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../s-rack_amd/csrc/jit_gen.hpp"

namespace srack {
int load_srk(const uint8_t* bytes, size_t n_bytes, Graph& g);  // srk.cpp
}
using namespace srack;

static unsigned long long fnv1a(const std::string& s)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    for (unsigned char ch : s) h = (h ^ ch) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv)
{
    uint32_t voices = 64, flags = 0, buffer = 1024;
    bool text = false;
    int mode = 3, waves = 0, ctl = -1;  // (--text: which combination; ctl -1 = with the control units where they can be generated, as the library's kernel_source)
    int n_files = 0;
    for (int i = 1; i < argc; i++) {
        const std::string arg = argv[i];
        auto value = [&]() -> const char* {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "jit_dump: %s needs a value\n", arg.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        if (arg == "--voices") voices = (uint32_t)std::strtoul(value(), nullptr, 0);
        else if (arg == "--flags") flags = (uint32_t)std::strtoul(value(), nullptr, 0);
        else if (arg == "--buffer") buffer = (uint32_t)std::strtoul(value(), nullptr, 0);
        else if (arg == "--mode") mode = std::atoi(value());
        else if (arg == "--waves") waves = std::atoi(value());
        else if (arg == "--ctl") { const char* v = value(); ctl = std::strcmp(v, "auto") == 0 ? -1 : std::atoi(v); }
        else if (arg == "--text") text = true;
        else {
            n_files++;
            std::ifstream f(arg, std::ios::binary);
            if (!f) {
                std::fprintf(stderr, "jit_dump: cannot read %s\n", arg.c_str());
                return 2;
            }
            const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            Graph g;
            g.cfg.sample_rate = 48000;
            g.cfg.buffer_size = buffer;
            g.cfg.channels = 2;
            FlatPair pair;
            // (SPECIALIZE / NO_SPECIALIZE choose a kernel for the same program: the library takes them out before it flattens, render.hip)
            const uint32_t program_flags = flags & ~(uint32_t)(SRACK_RENDER_SPECIALIZE | SRACK_RENDER_NO_SPECIALIZE);
            if (load_srk(bytes.data(), bytes.size(), g) != SRACK_OK || flatten(g, voices, {}, program_flags, pair) != SRACK_OK) {
                std::fprintf(stderr, "jit_dump: %s: %s\n", arg.c_str(), last_error());
                return 3;
            }
            std::string src;
            if (text) {
                const bool with_ctl = ctl < 0 ? jit_ctl_supported(pair) : ctl != 0;
                if (jit_source(pair, mode, with_ctl, src, 0, waves) != SRACK_OK) {
                    std::printf("error: %s\n", last_error());
                    continue;
                }
                std::fwrite(src.data(), 1, src.size(), stdout);
                continue;
            }
            for (int m = 1; m <= 4; m++)
                for (int c = 0; c < 2; c++)
                    for (int w = 0; w <= 4; w += 2) {
                        std::printf("%s mode=%d ctl=%d waves=%d ", arg.c_str(), m, c, w);
                        if (jit_source(pair, m, c != 0, src, 0, w) == SRACK_OK)
                            std::printf("%016llx %zu\n", fnv1a(src), src.size());
                        else
                            std::printf("error: %s\n", last_error());
                    }
        }
    }
    if (n_files == 0) {
        std::fprintf(stderr, "usage: jit_dump [--voices V] [--flags F] [--buffer B] [--text [--mode M] [--ctl 0|1|auto] [--waves W]] file.srk ...\n");
        return 2;
    }
    return 0;
}
