// dump_codegen_cases.cpp -- generator inputs that only executors with a device ever set (a measured conjunct order,
// hash-partition counts other than 64 with their bucket shift, records instead of lines): fills CodegenInput by hand,
// calls qe::generate_fused_source and writes the source of every case to <out dir>/<case>.hip.  Never touches a device.
// Built by tools/dump_generated_sources.py against a checkout's libqe_hip.so and qe_internal.h.
#include "qe_internal.h"

#include <cstdio>
#include <fstream>

using namespace qe;

static Expr column(int col, int type) {
    Expr e;
    Node n;
    n.kind = N_COLUMN;
    n.col = col;
    n.type = type;
    e.nodes.push_back(n);
    e.root = 0;
    e.program = {1, (uint8_t)type, (uint8_t)col};
    return e;
}

// col < lit (a DOUBLE column), appended to `e`; returns the node id
static int less_than(Expr &e, int col, double lit) {
    Node c, l, f;
    c.kind = N_COLUMN; c.col = col; c.type = QE_DOUBLE;
    l.kind = N_NUM; l.num = lit; l.type = QE_DOUBLE;
    e.nodes.push_back(c);
    e.nodes.push_back(l);
    f.kind = N_FN; f.fn = QE_FN_CMP_LT; f.type = QE_BOOLEAN;
    f.ops = {(int)e.nodes.size() - 2, (int)e.nodes.size() - 1};
    e.nodes.push_back(f);
    return (int)e.nodes.size() - 1;
}

static int and_of(Expr &e, int a, int b) {
    Node f;
    f.kind = N_FN; f.fn = QE_FN_AND; f.type = QE_BOOLEAN;
    f.ops = {a, b};
    e.nodes.push_back(f);
    return (int)e.nodes.size() - 1;
}

static void write_case(const std::string &dir, const std::string &name, const CodegenInput &in) {
    std::ofstream f(dir + "/" + name + ".hip");
    try {
        f << generate_fused_source(in).source;
    } catch (const Error &err) {
        f << "ERROR " << err.code << " " << err.msg << "\n";
    }
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s OUT_DIR\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    // a three-conjunct filter (a < 100 AND b < 0.5 AND c < 7) over DOUBLE columns, projections a and d, two measured orders
    {
        Expr filter;
        filter.root = and_of(filter, and_of(filter, less_than(filter, 0, 100.0), less_than(filter, 1, 0.5)), less_than(filter, 2, 7.0));
        Expr pa = column(0, QE_DOUBLE), pd = column(3, QE_DOUBLE);
        const std::vector<std::vector<int>> orders = {{2, 0, 1}, {1, 2, 0}};
        for (size_t o = 0; o < orders.size(); o++) {
            CodegenInput in;
            in.filter = &filter;
            in.projections = {&pa, &pd};
            for (int c = 0; c < 4; c++) in.schema.push_back(BoundColumn{QE_DOUBLE, c == 1, nullptr});
            in.conj_order = orders[o];
            write_case(dir, "conj_order_" + std::to_string(o), in);
        }
    }
    // hash-partitioned GROUP BY: one DOUBLE key / two INT64 keys, SUM + MIN of a DOUBLE value
    for (int nkeys = 1; nkeys <= 2; nkeys++)
        for (int nullable = 0; nullable <= 1; nullable++)
            for (int parts : {2, 256, 512, 1024})
                for (int shift : {6, 8, 12})
                    for (int lines = 0; lines <= 1; lines++) {
                        const int kt = nkeys == 1 ? QE_DOUBLE : QE_INT64;
                        Expr k0 = column(0, kt), k1 = column(1, kt), v = column(2, QE_DOUBLE);
                        CodegenInput in;
                        in.group_keys = {&k0};
                        if (nkeys == 2) in.group_keys.push_back(&k1);
                        in.projections = {&v, &v};
                        in.agg_fns = {QE_AGG_SUM, QE_AGG_MIN};
                        in.schema = {BoundColumn{kt, nullable != 0, nullptr}, BoundColumn{kt, false, nullptr}, BoundColumn{QE_DOUBLE, nullable != 0, nullptr}};
                        in.hp_parts = parts;
                        in.hp_shift = shift;
                        in.hp_lines = lines;
                        in.geo.threads = 512;
                        in.geo.unroll = 4;
                        write_case(dir, "hp_k" + std::to_string(nkeys) + (nullable ? "n" : "v") + "_p" + std::to_string(parts) + "_s" + std::to_string(shift) +
                                            "_l" + std::to_string(lines), in);
                    }
    return 0;
}
