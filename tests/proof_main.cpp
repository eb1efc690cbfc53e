// Stand-alone host check of reth_amd/csrc/proof_host.h against cases the
// Python side derived from oracle/pyref.py (built and run by
// tests/test_proof_host_cpu.py). The case file is one record per line,
// fields separated by blanks, bytes as hex ("-" = empty):
//   N                      start a new trie: forget the node universe
//   U node                 add a node to the universe
//   K msg hash             h_keccak256(msg) == hash
//   W root key present n node*n
//                          the walk over the universe emits exactly these
//   L key from nonce balance code_hash storage_root want     h_leaf_node
//   S slot from value want                                   h_storage_leaf
//   E key0 P d child want                                    h_row_ext
//   A root key present nrows (key0 P d rlp)*nrows nleaves leaf*nleaves
//     n node*n             proof_assemble, then one length / one byte short
//   X node                 h_rlp_list_items: whole, cut by 1, cut to half
//   M node key             the walk from this node fails as "malformed node"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "proof_host.h"

typedef std::vector<uint8_t> bytes;

static long n_checked = 0, n_failed = 0;

static void check(bool ok, const char *what, long line)
{
    ++n_checked;
    if (!ok && n_failed++ < 10)
        fprintf(stderr, "line %ld: %s\n", line, what);
}

static bytes unhex(const std::string &s)
{
    bytes b;
    if (s == "-")
        return b;
    auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2)
        b.push_back((uint8_t)(v(s[i]) << 4 | v(s[i + 1])));
    return b;
}

static bytes hex_tok(std::istringstream &in)
{
    std::string s;
    in >> s;
    return unhex(s);
}

static long int_tok(std::istringstream &in)
{
    long v = 0;
    in >> v;
    return v;
}

static std::vector<bytes> list_tok(std::istringstream &in)
{
    std::vector<bytes> v(int_tok(in));
    for (auto &b : v)
        b = hex_tok(in);
    return v;
}

// a copy in a heap block of exactly its size, so any read or write past it
// is an AddressSanitizer report
template <typename T> static std::unique_ptr<T[]> exact(size_t n)
{
    return std::unique_ptr<T[]>(new T[n]);
}

static const char FULL[] = "proof_main: output capacity exceeded";

// proof_assemble into buffers of exactly cap_nodes bytes / cap_lens lengths
static int assemble(const bytes &root, const bytes &key,
                    const std::vector<const proof_row *> &rows,
                    const std::vector<bytes> &leaves, uint64_t cap_nodes,
                    uint64_t cap_lens, std::vector<bytes> &got,
                    const char **why)
{
    auto nodes = exact<uint8_t>(cap_nodes);
    auto lens = exact<uint32_t>(cap_lens);
    proof_sink out{nodes.get(), cap_nodes, lens.get(), cap_lens, FULL};
    uint32_t count = 0;
    int rc = proof_assemble(root.data(), key.data(), rows, leaves, out, &count,
                            why);
    got.clear();
    if (rc >= 0) {
        if (count != out.nl)
            return -2;
        uint64_t off = 0;
        for (uint32_t k = 0; k < count; ++k) {
            got.emplace_back(nodes.get() + off, nodes.get() + off + lens[k]);
            off += lens[k];
        }
        if (off != out.nb)
            return -2;
    }
    return rc;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1]);
    std::vector<bytes> universe;
    node_map byhash;
    std::string text;
    for (long line = 1; std::getline(f, text); ++line) {
        std::istringstream in(text);
        std::string op;
        in >> op;
        if (op == "N") {
            universe.clear();
            byhash.clear();
        } else if (op == "U") {
            universe.push_back(hex_tok(in));
            byhash.clear();
        } else if (op == "K") {
            bytes msg = hex_tok(in), want = hex_tok(in);
            auto m = exact<uint8_t>(msg.size());
            if (!msg.empty())
                memcpy(m.get(), msg.data(), msg.size());
            uint8_t h[32];
            h_keccak256(m.get(), msg.size(), h);
            check(want.size() == 32 && !memcmp(h, want.data(), 32), "keccak",
                  line);
        } else if (op == "W") {
            bytes root = hex_tok(in), key = hex_tok(in);
            long present = int_tok(in);
            std::vector<bytes> want = list_tok(in), got;
            if (byhash.empty())
                for (const auto &n : universe)
                    map_add(byhash, n.data(), (int)n.size());
            const char *why = nullptr;
            int rc = proof_walk_emit(
                root.data(), byhash, key.data(),
                [&](const uint8_t *n, int len) {
                    got.emplace_back(n, n + len);
                    return 0;
                },
                &why);
            check(rc == (present ? 0 : 1) && got == want, "walk", line);
        } else if (op == "L") {
            bytes key = hex_tok(in);
            long from = int_tok(in);
            sre_account_entry a{};
            memcpy(a.key, key.data(), 32);
            a.nonce = (uint64_t)int_tok(in);
            memcpy(a.balance, hex_tok(in).data(), 32);
            memcpy(a.code_hash, hex_tok(in).data(), 32);
            bytes sroot = hex_tok(in), want = hex_tok(in);
            auto dst = exact<uint8_t>(200); // the size sre_account_proof gives
            int n = h_leaf_node(dst.get(), a.key, (int)from, &a, sroot.data());
            check(bytes(dst.get(), dst.get() + n) == want, "account leaf", line);
        } else if (op == "S") {
            bytes slot = hex_tok(in);
            long from = int_tok(in);
            bytes value = hex_tok(in), want = hex_tok(in);
            auto dst = exact<uint8_t>(96); // the size sre_storage_proof gives
            int n = h_storage_leaf(dst.get(), slot.data(), (int)from,
                                   value.data());
            check(bytes(dst.get(), dst.get() + n) == want, "storage leaf", line);
        } else if (op == "E") {
            proof_row r{};
            memcpy(r.key0, hex_tok(in).data(), 32);
            r.P = (int16_t)int_tok(in);
            r.d = (int16_t)int_tok(in);
            bytes child = hex_tok(in), want = hex_tok(in), got;
            r.br_len = (uint32_t)child.size();
            memcpy(r.rlp, child.data(), child.size());
            h_row_ext(&r, got);
            check(got == want, "extension", line);
        } else if (op == "A") {
            bytes root = hex_tok(in), key = hex_tok(in);
            long present = int_tok(in);
            std::vector<proof_row> rows(int_tok(in));
            for (auto &r : rows) {
                memcpy(r.key0, hex_tok(in).data(), 32);
                r.P = (int16_t)int_tok(in);
                r.d = (int16_t)int_tok(in);
                bytes rlp = hex_tok(in);
                r.target = 0;
                r.s = 0;
                r.e = 1;
                r.br_len = (uint32_t)rlp.size();
                memcpy(r.rlp, rlp.data(), rlp.size());
            }
            std::vector<const proof_row *> rp;
            for (const auto &r : rows)
                rp.push_back(&r);
            std::vector<bytes> leaves = list_tok(in), want = list_tok(in), got;
            uint64_t total = 0;
            for (const auto &n : want)
                total += n.size();
            const char *why = nullptr;
            int rc = assemble(root, key, rp, leaves, total, want.size(), got,
                              &why);
            check(rc == (present ? 0 : 1) && got == want, "assemble", line);
            why = nullptr;
            rc = assemble(root, key, rp, leaves, total, want.size() - 1, got,
                          &why);
            check(rc == -1 && why == FULL, "assemble, one length short", line);
            why = nullptr;
            rc = assemble(root, key, rp, leaves, total - 1, want.size(), got,
                          &why);
            check(rc == -1 && why == FULL, "assemble, one byte short", line);
        } else if (op == "X") {
            bytes node = hex_tok(in);
            size_t cuts[3] = {node.size(), node.size() - 1, node.size() / 2};
            for (int c = 0; c < 3; ++c) {
                auto b = exact<uint8_t>(cuts[c]);
                memcpy(b.get(), node.data(), cuts[c]);
                std::vector<h_item> items;
                int rc = h_rlp_list_items(b.get(), (int)cuts[c], items);
                check(rc == (c == 0 ? 0 : -1), "list parse", line);
            }
        } else if (op == "M") {
            bytes node = hex_tok(in), key = hex_tok(in);
            node_map one;
            map_add(one, node.data(), (int)node.size());
            const char *why = "";
            int rc = proof_walk_emit(
                one.begin()->first.data(), one, key.data(),
                [](const uint8_t *, int) { return 0; }, &why);
            check(rc == -1 && !strcmp(why, "proof: malformed node"),
                  "malformed node", line);
        } else if (!op.empty()) {
            fprintf(stderr, "line %ld: unknown record %s\n", line, op.c_str());
            return 2;
        }
    }
    printf("checked %ld failed %ld\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
