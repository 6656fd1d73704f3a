// stand-in for the reference's include/ORBVocabulary.h (a typedef of DBoW2::TemplatedVocabulary there): adapter/KeyFrameDatabase.cc
// asks the vocabulary for its size() only
#ifndef CVSTUB_ORBVOCABULARY_H
#define CVSTUB_ORBVOCABULARY_H
namespace ORB_SLAM2 {
class ORBVocabulary
{
public:
    explicit ORBVocabulary(unsigned int nwords = 0) : m_nwords(nwords) {}
    unsigned int size() const { return m_nwords; }
private:
    unsigned int m_nwords;
};
}
#endif
