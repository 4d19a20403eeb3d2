// kfmap_tri_check -- kfm_first_observer of csrc/kfmap_ring.hpp (the first observer of triangulate_temporal! on the key-frame map) as a stand-alone host
// program: tests/test_kfmap_tri_host.py feeds it cases and holds the output to the numpy rule.  One case per input line:
//   R  mask  tag[0] .. tag[R - 1]      mask: the observer bits as an unsigned 64-bit decimal; tag[b] = key-frame id + 1 of slot b (0: empty)
// Output line: the slot kfm_first_observer returns.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <iostream>
#include "kfmap_ring.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int R = 0;
        unsigned long long mask = 0;
        in >> R >> mask;
        if (R < 1 || R > 64) { std::printf("bad R\n"); return 1; }
        // exactly R tags, on the heap: a routine that reads the tag of a bit at or above R is the sanitizer's
        int *tag = (int *)std::calloc(R, sizeof(int));
        for (int b = 0; b < R; b++) in >> tag[b];
        if (!in) { std::printf("bad line\n"); return 1; }
        std::printf("%d\n", kfm_first_observer(mask, tag, R));
        std::free(tag);
    }
    return 0;
}
