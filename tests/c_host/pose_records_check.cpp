// pose_records_check -- a stand-alone host of csrc/pose_records.hpp and csrc/layout.hpp (no HIP, no library): reads one command per line from
// stdin, doubles as hex floats, and prints the routine's results as hex floats (integers in decimal), one line per command.
//   a2p  X[6]          -> T[16]: the identity, then angles_to_pose
//   p2a3 Rt[12]        -> X[6]:  pose_to_angles<3> of a column-major 3 x 4 [R | t]
//   p2a4 T[16]         -> X[6]:  pose_to_angles<4> of a column-major 4 x 4 pose
//   take (size count)* -> per pair: take<T>(count)'s offset, bytes() and the layout's end, then take(count * size)'s offset and end on a second layout
//   offsets            -> the offsetof / sizeof values of P3POut, FPOut, PnPResult
// tests/test_pose_records_host.py drives it, once built plain and once with -fsanitize=address,undefined.
#include "pose_records.hpp"
#include "layout.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct E16 { double v[2]; };
struct E24 { double v[3]; };

template <class T> static void take_both(Layout &typed, Layout &raw, size_t count)
{
    const Region<T> r = typed.take<T>(count);
    const size_t at = raw.take(count * sizeof(T));
    static std::vector<char> block(1 << 20);
    if (r.off + r.bytes() > block.size() || (char *)r.at(block.data()) != block.data() + r.off) { fprintf(stderr, "at() does not bind the offset\n"); exit(2); }
    if (count) r.at(block.data())[count - 1] = T();                // the last element lies inside the region (the sanitizer build watches the block)
    printf("%zu %zu %zu %zu %zu ", r.off, r.bytes(), typed.size(), at, raw.size());
}

int main()
{
    char *line = nullptr; size_t cap = 0;
    while (getline(&line, &cap, stdin) > 0) {
        std::vector<std::string> tok;
        for (char *p = strtok(line, " \n"); p; p = strtok(nullptr, " \n")) tok.push_back(p);
        if (tok.empty()) continue;
        std::vector<double> a;
        for (size_t i = 1; i < tok.size(); i++) a.push_back(strtod(tok[i].c_str(), nullptr));
        const std::string &cmd = tok[0];
        auto need = [&](size_t n) { if (a.size() != n) { fprintf(stderr, "%s: %zu arguments, not %zu\n", cmd.c_str(), a.size(), n); exit(2); } };
        if (cmd == "a2p") {
            need(6);
            double T[16];
            for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
            angles_to_pose(a.data(), T);
            for (int k = 0; k < 16; k++) printf("%a ", T[k]);
        } else if (cmd == "p2a3" || cmd == "p2a4") {
            double X[6];
            if (cmd == "p2a3") { need(12); pose_to_angles<3>(a.data(), a.data() + 9, X); }
            else { need(16); pose_to_angles<4>(a.data(), a.data() + 12, X); }
            for (int k = 0; k < 6; k++) printf("%a ", X[k]);
        } else if (cmd == "take") {
            Layout typed, raw;
            for (size_t i = 0; i + 1 < a.size(); i += 2) {
                const int size = (int)a[i]; const size_t count = (size_t)a[i + 1];
                if (size == 1) take_both<unsigned char>(typed, raw, count);
                else if (size == 4) take_both<int32_t>(typed, raw, count);
                else if (size == 8) take_both<double>(typed, raw, count);
                else if (size == 16) take_both<E16>(typed, raw, count);
                else if (size == 24) take_both<E24>(typed, raw, count);
                else { fprintf(stderr, "take: element size %d\n", size); exit(2); }
            }
        } else if (cmd == "offsets") {
            printf("%zu %zu %zu %zu %zu %zu ", offsetof(P3POut, KP), offsetof(P3POut, Rt), offsetof(P3POut, err), offsetof(P3POut, n_inliers), offsetof(P3POut, best_iter), sizeof(P3POut));
            printf("%zu %zu %zu %zu %zu %zu ", offsetof(FPOut, P), offsetof(FPOut, E), offsetof(FPOut, err), offsetof(FPOut, n_inliers), offsetof(FPOut, best_iter), sizeof(FPOut));
            printf("%zu %zu %zu %zu %zu %zu %zu %zu", offsetof(PnPResult, X), offsetof(PnPResult, err_init), offsetof(PnPResult, err_final), offsetof(PnPResult, n_outliers),
                   offsetof(PnPResult, identity), offsetof(PnPResult, iters1), offsetof(PnPResult, iters2), sizeof(PnPResult));
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); exit(2); }
        printf("\n");
    }
    free(line);
    return 0;
}
