// Stand-alone driver for truncate_terms_split (csrc/qagg_format.h): reads a
// QAGG1 blob on stdin, cuts its first aggregation (kind 3) to split_size
// entries in the given order, writes the blob to stdout.
//
//   g++ -std=c++17 -O1 tools/qagg_truncate_main.cpp -o qagg_truncate
//   ./qagg_truncate SPLIT_SIZE [ORDER_TARGET [asc|desc]] < in.blob > out.blob
//
// ORDER_TARGET: "" (doc count), "_key", or "sub" / "sub.stat". For the last
// form a sub of kind 0 counts as an `avg`, one of kind 1 as a percentiles.
// tests/test_terms_percentiles_cpu.py pins with it that the per-term sketches
// travel with their terms through every branch of the cut.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../quickwit_amd/csrc/qagg_format.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s SPLIT_SIZE [ORDER_TARGET [asc|desc]]\n", argv[0]);
        return 2;
    }
    try {
        std::string in((std::istreambuf_iterator<char>(std::cin)),
                       std::istreambuf_iterator<char>());
        qw::IntermediateAggResults ir = qw::IntermediateAggResults::decode(
            (const uint8_t*)in.data(), in.size());
        qw::AggResult& r = ir.aggs.at(0);
        std::vector<qw::MetricAgg> subs(r.sub_names.size());
        for (size_t s = 0; s < subs.size(); ++s) {
            subs[s].name = r.sub_names[s];
            subs[s].kind = r.sub_kinds[s] == 1 ? qw::MetricAgg::PERCENTILES
                                               : qw::MetricAgg::AVG;
        }
        std::string target = argc > 2 ? argv[2] : "";
        bool asc = argc > 3 && std::string(argv[3]) == "asc";
        qw::truncate_terms_split(r, atoll(argv[1]), target, asc, &subs);
        std::string out = ir.encode();
        fwrite(out.data(), 1, out.size(), stdout);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
