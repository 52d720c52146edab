// test_shim_bin_large_k.cpp -- Search::VectorIndex<..., BinaryVector>::search of shim/HostShim.cpp with k beyond MSVS_MAX_K (the
// host asks the binary index for LIMIT 1000, k + deleted rows): a BinaryFLAT index built from FixedString chunks with ids, searched
// with every k the caller lists, with and without a filter bitmap, both metrics.  Inputs are written by
// tests/test_shim_bin_large_k.py, which compares what comes back with its numpy reference.
//   usage: test_shim_bin_large_k <dir>
//          reads  <dir>/{meta.txt (rows nbytes queries nbits k...), bx.bin, blabels.bin (i64), bq.bin, balive.bin (a byte per label)}
//          writes <dir>/bi_{ham,jac}_k<K>_{ids,dis}[_f].bin
#include <SearchIndex/VectorIndex.h>

#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using IS = Search::AbstractIStream;
using OS = Search::AbstractOStream;
using Bitmap = Search::DenseBitmap;
using BinaryVI = Search::VectorIndex<IS, OS, Bitmap, Search::DataType::BinaryVector>;

namespace
{

template <typename T>
std::vector<T> slurp(const std::string & path)
{
    std::ifstream f(path, std::ios::binary);
    std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(s.size() / sizeof(T));
    memcpy(v.data(), s.data(), v.size() * sizeof(T));
    return v;
}

template <typename T>
void dump(const std::string & path, const T * p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(p), (std::streamsize)(n * sizeof(T)));
}

// ---- the build feed: FixedString chunks + the part's row offsets as ids, like VIPartReader::readDataImpl
class BinReader : public Search::IndexSourceDataReader<bool>
{
public:
    BinReader(const std::vector<uint8_t> & x_, const std::vector<int64_t> & labels_, size_t n_, size_t nbytes_)
        : x(x_), labels(labels_), n(n_), nbytes(nbytes_)
    {
    }
    size_t numDataRead() const override { return pos; }
    size_t dataDimension() const override { return nbytes * 8; }
    bool eof() override { return pos == n; }
    void seekg(std::streamsize, std::ios::seekdir) override { throw std::runtime_error("seekg() is not implemented"); }
    std::shared_ptr<DataChunk> sampleData(size_t) override { return nullptr; }

protected:
    std::shared_ptr<DataChunk> readDataImpl(size_t m) override
    {
        m = std::min(m, n - pos);
        if (m == 0)
            return nullptr;
        bool * data = new bool[m * nbytes]; // one byte = 8 bits (VIPartReader.h:262-266)
        Search::idx_t * ids = new Search::idx_t[m];
        memcpy(data, x.data() + pos * nbytes, m * nbytes);
        for (size_t i = 0; i < m; i++)
            ids[i] = (Search::idx_t)labels[pos + i];
        auto chunk = std::make_shared<DataChunk>(data, m, nbytes * 8, [=]() { delete[] data; });
        chunk->setDataID(ids, [=]() { delete[] ids; });
        pos += m;
        return chunk;
    }

private:
    const std::vector<uint8_t> & x;
    const std::vector<int64_t> & labels;
    size_t n, nbytes, pos = 0;
};

}

int main(int argc, char ** argv)
{
    if (argc < 2)
        return 2;
    const std::string dir = argv[1];
    size_t n = 0, nbytes = 0, nq = 0, nbits = 0;
    std::vector<size_t> ks;
    {
        std::ifstream m(dir + "/meta.txt");
        m >> n >> nbytes >> nq >> nbits;
        for (size_t k; m >> k;)
            ks.push_back(k);
    }
    auto bx = slurp<uint8_t>(dir + "/bx.bin");
    auto labels = slurp<int64_t>(dir + "/blabels.bin");
    auto bq = slurp<uint8_t>(dir + "/bq.bin");
    auto balive = slurp<uint8_t>(dir + "/balive.bin");
    if (n == 0 || nbytes == 0 || bx.size() != n * nbytes || labels.size() != n || bq.size() != nq * nbytes || balive.size() != nbits || ks.empty())
    {
        std::cerr << "test_shim_bin_large_k: inconsistent inputs\n";
        return 2;
    }
    try
    {
        auto cancel = []() { return false; };
        for (const char * mname : {"Hamming", "Jaccard"})
        {
            const auto metric = Search::getMetricType(mname, Search::DataType::BinaryVector);
            const auto type = Search::getVectorIndexType("BinaryFLAT", Search::DataType::BinaryVector);
            Search::Parameters des;
            std::shared_ptr<BinaryVI> index = Search::createVectorIndex<IS, OS, Bitmap, Search::DataType::BinaryVector>(
                "b1", type, metric, nbytes * 8, n, des, 8, "cache/", cancel);
            index->setAddDataChunkSize(nbytes * 400); // several chunks
            BinReader reader(bx, labels, n, nbytes);
            index->build(&reader, 4, cancel);
            if (!index->ready() || index->numData() != n)
                throw std::runtime_error("binary build did not produce a ready index");
            auto queries = std::make_shared<Search::DataSet<bool>>(reinterpret_cast<bool *>(bq.data()), (int64_t)nq, (int64_t)(nbytes * 8));
            auto filter = std::make_shared<Bitmap>(nbits);
            for (size_t i = 0; i < nbits; i++)
                if (balive[i])
                    filter->set(i);
            const std::string tag = mname[0] == 'H' ? "ham" : "jac";
            for (size_t k : ks)
            {
                Search::Parameters sp;
                const std::string base = dir + "/bi_" + tag + "_k" + std::to_string(k);
                auto r1 = index->search(queries, (int32_t)k, sp, false, nullptr);
                dump(base + "_ids.bin", r1->getResultIndices(), nq * k);
                dump(base + "_dis.bin", r1->getResultDistances(), nq * k);
                auto r2 = index->search(queries, (int32_t)k, sp, false, filter.get());
                dump(base + "_ids_f.bin", r2->getResultIndices(), nq * k);
                dump(base + "_dis_f.bin", r2->getResultDistances(), nq * k);
            }
        }
    }
    catch (const std::exception & e)
    {
        std::cerr << "test_shim_bin_large_k failed: " << e.what() << "\n";
        return 1;
    }
    std::cout << "test_shim_bin_large_k ok\n";
    return 0;
}
