"""Generate tests/golden/en_report.json from the reference's recorded run.

Run ONCE where the reference's resources exist:

    python tests/golden/make_report_golden.py

Source: ``TestOutput/Result_EN_1591723228815``, the text LDALoader.scala writes.  Recorded per book (in the
file's order, which is en_topicdist.json's ``books``): its name, the printed main topic (LDALoader.scala:151)
and the "Book most important words" list (:161-164); per topic the "Amount of books in the topic" (the counts
of :142).  This is DATA the reference wrote; the tests read only the fixture.
"""
import json
import os
import re

REF = "/root/reference/TextClustering/src/main/resources"
OUT = os.path.dirname(os.path.abspath(__file__))
RUN = "Result_EN_1591723228815"


def main():
    lines = open(os.path.join(REF, "TestOutput", RUN), encoding="utf-8").read().split("\n")
    books, counts = [], []
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("Book's name: "):
            books.append({"name": ln[len("Book's name: "):]})
        m = re.match(r"Main topic of the book: Topic Nr\. \((\d+)\), Weight \((.*)\)$", ln)
        if m:
            books[-1]["main_topic"] = int(m.group(1))
            books[-1]["main_topic_weight"] = m.group(2)
        if ln.startswith("Word. \t|\t TF"):
            words = lines[i + 2]
            assert words == "" or words.endswith(", "), words
            books[-1]["words"] = [w for w in words.split(", ") if w]
            i += 2
        m = re.match(r"Amount of books in the topic: (\d+)$", ln)
        if m:
            counts.append(int(m.group(1)))
        i += 1
    assert all(set(b) == {"name", "main_topic", "main_topic_weight", "words"} for b in books)
    meta = json.load(open(os.path.join(OUT, "en_topicdist.json"), encoding="utf-8"))
    assert [b["name"] for b in books] == meta["books"]
    assert sum(counts) == len(books) and len(counts) == meta["k"]
    with open(os.path.join(OUT, "en_report.json"), "w", encoding="utf-8") as f:
        json.dump({"run": RUN, "doc_terms": 100, "topic_terms": 300, "n": 10, "books": books,
                   "books_per_topic": counts}, f, ensure_ascii=False, indent=1)
        f.write("\n")
    print(f"en_report.json: {len(books)} books, counts {counts}")


if __name__ == "__main__":
    main()
